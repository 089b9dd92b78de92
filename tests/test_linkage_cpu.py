"""Oracle restatement of moped3d's CLUSTER_LINKAGE_CPU (oracle/linkage_oracle.cpp): hand-worked
cases, and its agglomeration (orc_linkage_agglomerate) against the Python witness of tests/linkage_ref.py.  PARITY UNPINNED
against a reference build (CLUSTER_LINKAGE_CPU.hpp works on IplImage); the GPU kernel is compared with this oracle in
tests/test_gpu_linkage.py and, stage by stage, in tests/test_gpu_linkage_stages.py."""
import numpy as np

import orclib
from linkage_ref import agglomerate, flat_map, lattice, similarity_f64, world_of

K = np.array([800, 800, 320, 240], np.float32)


def _plane(z=1.0, h=480, w=640):
    v, u = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 4), np.float32)
    img[..., 0] = (u - K[2]) / K[0] * z
    img[..., 1] = (v - K[3]) / K[1] * z
    img[..., 2] = z
    img[..., 3] = np.sqrt((img[..., :3] ** 2).sum(-1))
    return img


def _world(img, uv):
    return img[uv[:, 1].astype(int), uv[:, 0].astype(int), :3].copy()


def test_similarity_matrix_on_a_flat_scene():
    """Flat depth: the discontinuity kernel is exp(0) = 1 off the diagonal and exp(1 / (-2 (pi/128)^2)) = 0 on
    it (a single Bresenham sample leaves maxAngleDiff at -1); model == world points make the
    distance-consistency kernel 1; measured pixels (fill distance 0) give w2D = w3D = 0.5."""
    img = _plane()
    uv = np.array([[100, 100], [110, 100], [100, 112], [400, 300]], np.float32)
    world = _world(img, uv)
    cl, Km = orclib.cluster_linkage(uv, world, world, img, np.zeros((480, 640), np.float32), min_pts=0, want_k=True)
    assert np.array_equal(Km, Km.T)
    # sigma2D = mean nearest-neighbour distance = (10 + 10 + 12 + |(400,300)-(110,100)|) / 4
    d = np.sqrt(((uv[:, None] - uv[None]) ** 2).sum(-1)); np.fill_diagonal(d, np.inf)
    s2 = np.float32(d.min(1).astype(np.float32).sum() / 4)
    dw = np.sqrt(((world[:, None] - world[None]) ** 2).sum(-1)); np.fill_diagonal(dw, np.inf)
    s3 = np.float32(dw.min(1).astype(np.float32).sum() / 4)
    k2 = np.exp(-((uv[0] - uv[1]) ** 2).sum() / (2 * s2 * s2))
    k3 = np.exp(-((world[0] - world[1]) ** 2).sum() / (2 * s3 * s3))
    # K3D + BK = k3 + 1, normalised by the matrix maximum (the largest off-diagonal k3 + 1), times K3F = 1, normalised again
    offd = [np.exp(-((world[i] - world[j]) ** 2).sum() / (2 * s3 * s3)) + 1 for i in range(4) for j in range(4) if i != j]
    want = 0.5 * k2 + 0.5 * (k3 + 1) / max(offd)
    assert abs(Km[0, 1] - want) < 1e-5
    assert abs(Km[0, 0] - (0.5 * 1 + 0.5 * 1 / max(offd))) < 1e-5     # diagonal: K2D = 1, K3D = 1 + 0
    # on a flat scene the discontinuity kernel alone keeps every similarity at 0.25 or more: with the
    # shipped cutoff (0.1) everything ends up in one cluster, the far point included
    assert Km.min() > 0.25 and [sorted(c.tolist()) for c in cl] == [[0, 1, 2, 3]]
    cl = orclib.cluster_linkage(uv, world, world, img, np.zeros((480, 640), np.float32), cutoff=0.5, min_pts=0)
    assert [sorted(c.tolist()) for c in cl] == [[0, 1, 2], [3]]


def test_member_order_and_min_pts():
    """Merging appends the absorbed cluster back to front; clusters need MORE than MinPts members."""
    img = _plane()
    img[:, 320:, :3] *= 3.0                                             # a 2 m depth step between the two groups
    rng = np.random.default_rng(3)
    a = rng.uniform([100, 100], [140, 140], (9, 2)).astype(np.float32)
    b = rng.uniform([400, 300], [440, 340], (8, 2)).astype(np.float32)
    uv = np.concatenate([a, b])
    world = _world(img, uv)
    cl = orclib.cluster_linkage(uv, world, world, img, None)            # MinPts 7 -> both groups (9 and 8 > 7)
    assert [sorted(c.tolist()) for c in cl] == [list(range(9)), list(range(9, 17))]
    assert cl[0][0] == 0 and cl[1][0] == 9                              # a cluster starts with its lowest index
    assert not np.array_equal(cl[0], np.sort(cl[0]))                    # ... and is not in index order
    cl8 = orclib.cluster_linkage(uv, world, world, img, None, min_pts=8)
    assert [sorted(c.tolist()) for c in cl8] == [list(range(9))]        # 8 is not MORE than 8
    # a high cutoff leaves every point alone, and singletons are not clusters
    assert orclib.cluster_linkage(uv, world, world, img, None, cutoff=2.0) == []
    assert [len(c) for c in orclib.cluster_linkage(uv, world, world, img, None, cutoff=2.0, min_pts=0)] == [1] * 17


def test_depth_discontinuity_separates_what_the_image_joins():
    """Two groups next to each other in the image but 0.5 m apart in depth, with a depth step
    between them: the discontinuity and 3-D kernels keep them apart."""
    img = _plane(1.0)
    img[:, 320:, :3] *= 1.5
    rng = np.random.default_rng(5)
    a = rng.uniform([280, 200], [315, 240], (10, 2)).astype(np.float32)
    b = rng.uniform([325, 200], [360, 240], (10, 2)).astype(np.float32)
    uv = np.concatenate([a, b])
    world = _world(img, uv)
    cl = orclib.cluster_linkage(uv, world, world, img, None)
    assert [sorted(c.tolist()) for c in cl] == [list(range(10)), list(range(10, 20))]
    flat = _plane(1.0)
    cl = orclib.cluster_linkage(uv, _world(flat, uv), _world(flat, uv), flat, None)
    assert [sorted(c.tolist()) for c in cl] == [list(range(20))]        # same image points on a flat scene: one cluster


def test_degenerate_inputs():
    img = _plane()
    assert orclib.cluster_linkage(np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), img, None) == []
    one = np.array([[10, 10]], np.float32)
    assert orclib.cluster_linkage(one, _world(img, one), _world(img, one), img, None, min_pts=0)[0].tolist() == [0]
    same = np.array([[10.2, 10.7]] * 9, np.float32)        # identical pixels: sigma = 0, similarities NaN/0 -> no merges
    assert orclib.cluster_linkage(same, _world(img, same), _world(img, same), img, None) == []


def test_minimum_and_maximum_linkage_against_an_independent_agglomeration():
    """LinkageType 0 / 2 (CLUSTER_LINKAGE_CPU.hpp:506-507, :525; the shipped configuration uses 1): the oracle's clusters,
    members in its order, equal a from-scratch agglomeration over the oracle's own similarity matrix."""
    img = _plane()
    img[:, 320:, :3] *= 2.0
    rng = np.random.default_rng(11)
    uv = np.concatenate([rng.uniform([60, 60], [200, 200], (14, 2)), rng.uniform([380, 250], [520, 400], (12, 2)),
                         rng.uniform([0, 0], [639, 479], (6, 2))]).astype(np.float32)
    world = _world(img, uv)
    fill = np.zeros((480, 640), np.float32)
    seen = set()
    for ltype in (0, 2):
        for cutoff in (0.05, 0.2, 0.45, 0.7):
            got, Km = orclib.cluster_linkage(uv, world, world, img, fill, cutoff=cutoff, min_pts=1, linkage_type=ltype, want_k=True)
            want, _ = agglomerate(Km, cutoff, 1, ltype)        # tests/linkage_ref.py
            assert [c.tolist() for c in got] == want, (ltype, cutoff)
            seen.add((ltype, len(want)))
    assert len({n for _, n in seen}) >= 2            # the cutoffs do produce different partitions
    # minimum linkage merges no further than maximum linkage at the same cutoff
    n0 = len(orclib.cluster_linkage(uv, world, world, img, fill, cutoff=0.45, min_pts=0, linkage_type=0))
    n2 = len(orclib.cluster_linkage(uv, world, world, img, fill, cutoff=0.45, min_pts=0, linkage_type=2))
    assert n0 >= n2


# ---- the agglomeration on its own: orc_linkage_agglomerate against the Python witness (tests/linkage_ref.py) ----------

def _lattice_matrix(n=36):
    img = flat_map()
    uv = lattice(n)
    world = world_of(img, uv)
    _, Km = orclib.cluster_linkage(uv, world, world, img, np.zeros((480, 640), np.float32), min_pts=0, want_k=True)
    return Km


def _same_clusters(Km, cutoff, min_pts, ltype):
    got = orclib.linkage_agglomerate(Km, cutoff, min_pts, ltype)
    want, stats = agglomerate(Km, cutoff, min_pts, ltype)
    assert [c.tolist() for c in got] == want, (len(Km), cutoff, min_pts, ltype)
    return want, stats


def test_lattice_ties_drive_the_list_handling():
    """6 x 6 pixel lattice on a flat map: few distinct similarities among the pairs, so every merge is decided by "first
    maximum in scan order", and at cutoff 0.3 average and minimum linkage win about every second merge through the stale
    row of the index absorbed just before.  The input must keep doing that; the oracle equals the witness for all three
    types, members in order."""
    Km = _lattice_matrix(36)
    assert np.array_equal(Km, Km.T)
    off = Km[np.triu_indices(36, 1)]
    assert len(np.unique(off)) <= 40 and len(off) == 630
    for ltype in (0, 1, 2):
        for cutoff in (0.3, 0.45, 0.6):
            want, stats = _same_clusters(Km, cutoff, 0, ltype)
            if cutoff == 0.3 and ltype in (0, 1):
                print(ltype, stats)
                assert stats["stale"] >= 30 and stats["merges"] >= 2 * 36 - 4 and stats["skipped"] >= 20, stats
    # one body: the whole oracle call gives what its agglomeration gives on its own matrix
    img, uv = flat_map(), lattice(36)
    world = world_of(img, uv)
    whole = orclib.cluster_linkage(uv, world, world, img, None, cutoff=0.3, min_pts=2)
    _, Km2 = orclib.cluster_linkage(uv, world, world, img, None, min_pts=0, want_k=True)
    assert [c.tolist() for c in whole] == [c.tolist() for c in orclib.linkage_agglomerate(Km2, 0.3, 2, 1)]


def three_valued(n, seed):
    """Random symmetric matrix over {0.2, 0.5, 0.8}: ties everywhere, no structure."""
    rng = np.random.default_rng([n, seed])
    M = rng.choice(np.array([0.2, 0.5, 0.8], np.float32), (n, n))
    M = np.triu(M) + np.triu(M, 1).T
    return np.ascontiguousarray(M, np.float32)


def test_agglomeration_on_random_and_degenerate_matrices():
    for n in (2, 3, 17, 40):
        for seed in range(3):
            M = three_valued(n, seed)
            for ltype in (0, 1, 2):
                for cutoff in (0.1, 0.4, 0.7):
                    _same_clusters(M, cutoff, 0, ltype)
    # NaN entries (never a maximum, never a minimum) and rows entirely below the cutoff
    rng = np.random.default_rng(7)
    for n in (5, 17, 33):
        M = three_valued(n, 9)
        hole = np.triu(rng.random((n, n)) < 0.3, 1)
        M[hole | hole.T] = np.nan
        M[n // 2, :] = M[:, n // 2] = 0.05
        M[0, :] = M[:, 0] = np.nan
        for ltype in (0, 1, 2):
            for cutoff in (0.1, 0.4):
                want, _ = _same_clusters(M, cutoff, 0, ltype)
                assert [n // 2] in want                         # below the cutoff: left alone
                # all NaN: left alone too -- except under minimum linkage, where a merged cluster's minimum over nothing
                # but NaN stays at its start value 1e20 (:404-413), the largest "similarity" of the next scan
                assert ([0] in want) == (ltype != 0), (n, ltype, cutoff)
    # min_pts counts strictly: a cluster of min_pts members is none, of min_pts + 1 it is one
    M = np.full((7, 7), 0.1, np.float32)
    M[:4, :4] = 0.9
    M[4:, 4:] = 0.9
    assert [len(c) for c in _same_clusters(M, 0.5, 3, 1)[0]] == [4]
    assert [len(c) for c in _same_clusters(M, 0.5, 2, 1)[0]] == [4, 3]
    assert _same_clusters(M, 0.5, 4, 1)[0] == []


def test_float64_restatement_has_the_oracles_nan_mask():
    """tests/linkage_ref.py similarity_f64 against the oracle's matrices: equal NaN masks, and values within float32
    rounding of each other on a scene with a depth step, fill distances, identical pixels and identical model points."""
    img = flat_map()
    img[:, 320:, :3] *= 1.5
    img[200:210, 100:110, 2] = np.nan
    rng = np.random.default_rng(4)
    uv = rng.uniform([0, 0], [639, 479], (40, 2)).astype(np.float32)
    uv[5] = uv[4]                                               # identical pixels: K3F is 0 / 0 there
    uv[7] = (104.5, 204.5)                                      # a NaN depth
    fill = (rng.uniform(0, 30, (480, 640)) * (rng.random((480, 640)) < 0.5)).astype(np.float32)
    world = world_of(img, uv)
    mx = (world + rng.normal(0, 0.01, world.shape)).astype(np.float32)
    mx[9] = mx[8]                                               # identical model points: K3F divides by zero
    for use3d in (0, 1, 2):
        for sig in ((-1.0, -1.0), (15.0, 0.05)):
            _, Ko, Ao = orclib.cluster_linkage(uv, mx, world, img, fill, use3d_filter=use3d, sigma2d=sig[0], sigma3d=sig[1],
                                               want_k=True, want_a=True)
            A64, K64 = similarity_f64(uv, mx, world, img, fill, use3d, *sig)
            assert np.array_equal(np.isnan(Ko), np.isnan(K64)) and np.array_equal(np.isnan(Ao), np.isnan(A64)), (use3d, sig)
            assert np.isnan(Ko).any() and not np.isnan(Ko).all()
            ok = ~np.isnan(Ko)
            assert np.abs(Ko[ok] - K64[ok]).max() < 1e-4, (use3d, sig, np.abs(Ko[ok] - K64[ok]).max())
