"""MH_LINKAGE_ROWMAX (mh_linkage_set_mode; moped_amd/csrc/linkage_rowmax.hip): the linkage clusterer with the matrix
stage on the whole grid and the merge loop over cached row maxima -- the same bytes as the default mode
(MH_LINKAGE_SCAN, linkage.hip), for lists of up to 4096 matches.  Inputs are tests/test_gpu_linkage_stages.py's.

1. MODES AGREE: every family at 1, 2, 3, 17, 45, 64, 65, 129, 160, 161, 257, 1024 points: A and K equal as uint32,
   clusters, member order and labels equal; linkage_stats counts the problems in ROWMAX only.
2. BEYOND 1024: "scene" at 1025 and 1500, average linkage: the matrix against the oracle and the float64 restatement
   with the stages file's bound e_dev <= max(4 e_ref, 2^-21) (the restatement takes 2.5 s / 5 s on the CPU at these
   sizes), the clusters equal orc_linkage_agglomerate(K_device) exactly; SCAN refuses the same call (MH_ERR_CAPACITY).
3. GIVEN MATRICES through linkage_debug_agglomerate: ties, NaN and blocks at 2 .. 1025 rows, all three linkage types, and
   4096 rows of block structure with fewer than 100 merges; exact.
4. THE CAP THROUGH THE MATRIX STAGE: 4096 "scene" points, a cutoff that leaves a few dozen merges: K bit-symmetric, its NaN
   mask A's, clusters the oracle's on K_device.
5. FRAME FORM: the stages file's 20-model frame; a frame with a list of about 1200 matches beside lists of 0, <= MinPts
   and > 160; a merged batch of three such frames, twice.
6. ERRORS AND STATE.  7. HOSTS: moped3d_hip_test --linkage-rowmax."""
import os
import time

import numpy as np
import pytest

import linkage_ref as ref
import orclib
import test_gpu_host_moped3d as host3d
import test_gpu_linkage_stages as stages
from moped_amd import capi, synth
from test_gpu_linkage_stages import FAMILIES, case_params, family_case, frames  # noqa: F401  (frames: the fixture)

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
W, H = stages.W, stages.H
SCAN, ROWMAX = capi.LINKAGE_SCAN, capi.LINKAGE_ROWMAX
ERR_MS_CAP = 1
SIZES = (1, 2, 3, 17, 45, 64, 65, 129, 160, 161, 257, 1024)


@pytest.fixture(scope="module")
def device():
    d = stages.Device()
    yield d
    d.c.linkage_set_mode(SCAN)
    d.close()


def lists(clusters):
    return [c.tolist() for c in clusters]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1: the modes agree -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_modes_agree(device, n):
    c = device.c
    for family in FAMILIES:
        name, uv, mx, world = family_case(family, n, device.maps)
        use3d, sig, ltype, cutoff, min_pts = case_params(family, n)
        tag = (family, n, use3d, sig, ltype, cutoff, min_pts)
        device.use(name)
        prm = capi.mh_linkage_params(cutoff, min_pts, use3d, sig[0], sig[1], ltype)
        got = {}
        for mode in (SCAN, ROWMAX):
            c.linkage_set_mode(mode)
            c.linkage_stats(reset=True)
            A, Km = c.linkage_debug_matrix(uv, mx, world, prm)
            (clusters, label), = c.cluster_linkage([(uv, mx, world)], prm)
            got[mode] = (A, Km, clusters, label, c.linkage_stats())
        c.linkage_set_mode(SCAN)
        (A0, K0, cl0, lab0, st0), (A1, K1, cl1, lab1, st1) = got[SCAN], got[ROWMAX]
        assert np.array_equal(bits(K0), bits(K1)), (tag, "K")
        assert np.array_equal(bits(A0), bits(A1)), (tag, "A")
        assert lists(cl0) == lists(cl1), tag
        assert np.array_equal(lab0, lab1), tag
        assert st0 == (0, 0, 0, 0), (tag, st0)
        assert st1[0] == 2 and st1[3] == n, (tag, st1)      # (the matrix call and the clustering call)


# ---- 2: beyond 1024 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1025, 1500))
def test_beyond_1024(device, n):
    c = device.c
    name, uv, mx, world = family_case("scene", n, device.maps)
    img, fill = device.maps[name]
    device.use(name)
    cutoff, min_pts, use3d = 0.3, 3, 2
    prm = capi.mh_linkage_params(cutoff, min_pts, use3d, -1.0, -1.0, 1)
    c.linkage_set_mode(SCAN)
    with pytest.raises(capi.MhError, match="more than 1024"):
        c.cluster_linkage([(uv, mx, world)], prm)
    with pytest.raises(capi.MhError, match="1 .. 1024"):
        c.linkage_debug_matrix(uv, mx, world, prm)
    c.linkage_set_mode(ROWMAX)
    try:
        A_dev, K_dev = c.linkage_debug_matrix(uv, mx, world, prm)
        (clusters, label), = c.cluster_linkage([(uv, mx, world)], prm)
    finally:
        c.linkage_set_mode(SCAN)
    t0 = time.perf_counter()
    _, K_orc, A_orc = orclib.cluster_linkage(uv, mx, world, img, fill, use3d_filter=use3d, want_k=True, want_a=True)
    t1 = time.perf_counter()
    A64, K64 = ref.similarity_f64(uv, mx, world, img, fill, use3d, -1.0, -1.0)
    t2 = time.perf_counter()
    for what, dev_m, orc_m, f64_m in (("K", K_dev, K_orc, K64), ("A", A_dev, A_orc, A64)):
        nan = np.isnan(orc_m)
        assert np.array_equal(np.isnan(dev_m), nan), (n, what, "NaN mask")
        assert np.array_equal(np.isnan(f64_m), nan), (n, what, "NaN mask of the float64 restatement")
        assert np.array_equal(bits(dev_m), bits(dev_m.T)), (n, what, "not symmetric bit for bit")
        ok = ~nan
        e_ref = float(np.abs(orc_m[ok].astype(np.float64) - f64_m[ok]).max())
        e_dev = float(np.abs(dev_m[ok].astype(np.float64) - f64_m[ok]).max())
        scale = 1.0 if what == "K" else float(np.abs(f64_m[ok]).max())
        print(n, what, "e_ref %.3g e_dev %.3g floor %.3g" % (e_ref, e_dev, stages.FLOOR * scale))
        assert e_dev <= max(4 * e_ref, stages.FLOOR * scale), (n, what, e_ref, e_dev)
    want = orclib.linkage_agglomerate(K_dev, cutoff, min_pts, 1)
    t3 = time.perf_counter()
    print(n, "oracle matrix %.1f s, float64 %.1f s, oracle merge loop %.1f s; %d clusters" % (t1 - t0, t2 - t1, t3 - t2, len(want)))
    assert lists(clusters) == lists(want) and len(want) >= 1
    assert np.array_equal(label, stages._labels(n, want))


# ---- 3: given matrices ------------------------------------------------------------------------------------------------------

def blocks(n, seed=0):
    rng = np.random.default_rng([0xB10C, n, seed])
    g = rng.integers(0, max(1, n // 8) + 1, n)
    M = (np.where(g[:, None] == g[None, :], 0.7, 0.1) + rng.uniform(-0.08, 0.08, (n, n))).astype(np.float32)
    return np.ascontiguousarray(np.triu(M) + np.triu(M, 1).T, np.float32)


def given_matrix(name, n):
    if name == "ties":
        return stages.three_valued(n, 1)
    if name == "blocks":
        return blocks(n)
    holes = stages.three_valued(n, 2)
    hole = np.triu(np.random.default_rng(n).random((n, n)) < 0.3, 1)
    holes[hole | hole.T] = np.nan
    holes[0, :] = holes[:, 0] = np.nan
    return holes


@pytest.mark.parametrize("n", (2, 3, 64, 65, 129, 257, 1025))
@pytest.mark.parametrize("name", ("ties", "nan", "blocks"))
def test_given_matrices(device, name, n):
    c = device.c
    M = given_matrix(name, n)
    cutoffs = (0.3, 0.6) if n < 1025 else (0.6,)         # (the oracle's merge loop is cubic: 1 .. 4 s per run at 1025)
    c.linkage_set_mode(ROWMAX)
    try:
        merged = 0
        for ltype in (0, 1, 2):
            for cutoff in cutoffs:
                clusters, label = c.linkage_debug_agglomerate(M, cutoff, 0, ltype)
                want = orclib.linkage_agglomerate(M, cutoff, 0, ltype)
                assert lists(clusters) == lists(want), (n, name, ltype, cutoff)
                assert np.array_equal(label, stages._labels(n, want)), (n, name, ltype, cutoff)
                merged += len(want) < n
        assert merged >= 2 or n <= 3        # (two or three rows: nothing but NaN, or no pair of one block)
    finally:
        c.linkage_set_mode(SCAN)


@pytest.mark.parametrize("ltype", (1, 0))
def test_given_matrix_of_4096_rows(device, ltype):
    """Block structure that leaves few merges: 40 groups of 3 rows at ~0.8, everything else ~0.1, cutoff 0.5 (the oracle's
    merge loop: 3 .. 4 s on the CPU)."""
    n = capi.LINKAGE_MAX_POINTS
    rng = np.random.default_rng(4096)
    M = rng.uniform(0.05, 0.15, (n, n)).astype(np.float32)
    rows = rng.choice(n, 120, replace=False).reshape(40, 3)
    rows[0] = (n - 3, n - 2, n - 1)                        # (the last rows among them)
    for g in rows:
        M[np.ix_(g, g)] = rng.uniform(0.75, 0.85, (3, 3)).astype(np.float32)
    M = np.ascontiguousarray(np.triu(M) + np.triu(M, 1).T, np.float32)
    c = device.c
    c.linkage_set_mode(ROWMAX)
    try:
        c.linkage_stats(reset=True)
        clusters, label = c.linkage_debug_agglomerate(M, 0.5, 1, ltype)
        stats = c.linkage_stats()
        t0 = time.perf_counter()
        want = orclib.linkage_agglomerate(M, 0.5, 1, ltype)
        print("4096 rows, type", ltype, "oracle %.1f s" % (time.perf_counter() - t0), "stats", stats)
        assert lists(clusters) == lists(want)
        assert sorted(len(x) for x in want) == [3] * 40 and 80 <= stats[1] < 200 and stats[3] == n
        assert np.array_equal(label, stages._labels(n, want))
    finally:
        c.linkage_set_mode(SCAN)


# ---- 4: the cap through the matrix stage -------------------------------------------------------------------------------------

def test_4096_points_through_the_matrix_stage(device):
    n = capi.LINKAGE_MAX_POINTS
    c = device.c
    name, uv, mx, world = family_case("scene", n, device.maps)
    device.use(name)
    c.linkage_set_mode(ROWMAX)
    try:
        prm = capi.mh_linkage_params(0.1, 0, 2, -1.0, -1.0, 1)
        A, Km = c.linkage_debug_matrix(uv, mx, world, prm)
        assert np.array_equal(bits(Km), bits(Km.T)), "K not symmetric bit for bit"
        assert np.array_equal(np.isnan(Km), np.isnan(A)), "K's NaN mask is not A's"
        assert np.isnan(Km).mean() < 0.5
        # a cutoff between the 40th and 41st largest similarity above the diagonal: a few dozen merges
        upper = Km[np.triu_indices(n, 1)]
        top = np.sort(np.unique(upper[~np.isnan(upper)]))[::-1]
        cutoff = float(np.float32((np.float64(top[39]) + np.float64(top[40])) / 2))
        prm = capi.mh_linkage_params(cutoff, 0, 2, -1.0, -1.0, 1)
        c.linkage_stats(reset=True)
        (clusters, label), = c.cluster_linkage([(uv, mx, world)], prm)
        stats = c.linkage_stats()
        t0 = time.perf_counter()
        want = orclib.linkage_agglomerate(Km, cutoff, 0, 1)
        print("4096 points: cutoff %.6f, oracle %.1f s, stats %s, largest cluster %d" %
              (cutoff, time.perf_counter() - t0, stats, max(len(x) for x in want)))
        assert lists(clusters) == lists(want)
        assert np.array_equal(label, stages._labels(n, want))
        assert 10 <= stats[1] < 200 and stats[3] == n and len(want) < n
    finally:
        c.linkage_set_mode(SCAN)


# ---- 5: the frame form ---------------------------------------------------------------------------------------------------------

def test_frame_form_table_equals_scans(frames):
    """The stages file's 20-model frame: the ROWMAX cluster table is SCAN's (and the oracle's)."""
    w = frames
    c = w.context(stages.Q_FRAME)
    try:
        scan = w.alone(c, 0)
        c.linkage_set_mode(ROWMAX)
        c.linkage_stats(reset=True)
        rowmax = w.alone(c, 0)
        assert rowmax[3] == scan[3] == w.tables[0]
        assert np.array_equal(rowmax[1], scan[1]) and rowmax[0].tobytes() == scan[0].tobytes()
        busy = sum(len(l[0]) > w.prm.min_pts for l in w.lists[0])
        stats = c.linkage_stats()
        assert stats[0] == busy and stats[3] == max(len(l[0]) for l in w.lists[0]), stats
        assert c.frame_counters()["error"] == 0
        assert w.alone(c, 0)[3] == scan[3]                       # again on the same context
        c.linkage_set_mode(SCAN)
        assert w.alone(c, 0)[3] == scan[3]
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()


Q_BIG = 2048
# matches planted per model: one list beyond 1024, lists of 0 and of 1 .. MinPts, one beyond the LDS matrix's 160 rows
PLANTED_BIG = (1200, 0, 5, 200, 40, 7)


def big_frame(db, planted, seed):
    """planted[m] features that match rows of model m (the rows' descriptors + noise) at pixels in a patch of the image,
    clutter that matches nothing.  The pixels are not the points' projections: CLUSTER does not ask."""
    rng = np.random.default_rng([0xB16, seed])
    descs, uvs = [], []
    for m, k in enumerate(planted):
        rows = rng.choice(np.nonzero(db.model_of == m)[0], size=k, replace=False)
        d = db.desc[rows] + rng.normal(0, 0.01, (k, 128)).astype(np.float32)
        descs.append(synth.l2_normalize(np.maximum(d, 0).astype(np.float32)))
        u0, v0 = rng.uniform(150, W - 150), rng.uniform(120, H - 120)
        uvs.append(rng.uniform([u0 - 100, v0 - 80], [u0 + 100, v0 + 80], (k, 2)).astype(np.float32))
    n_clutter = Q_BIG - sum(planted)
    descs.append(synth.l2_normalize(np.abs(rng.normal(size=(n_clutter, 128))).astype(np.float32)))
    uvs.append(rng.uniform([0, 0], [W, H], (n_clutter, 2)).astype(np.float32))
    perm = rng.permutation(Q_BIG)
    return np.ascontiguousarray(np.concatenate(descs)[perm]), np.ascontiguousarray(np.concatenate(uvs)[perm])


class BigWorld:
    def __init__(self, frames_world):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.db = synth.make_db(len(PLANTED_BIG), 1500, seed=12)
        self.dbn = orclib.normalize(self.db.desc)
        self.prm = capi.default_linkage_params()
        rot = lambda k: PLANTED_BIG[k:] + PLANTED_BIG[:k]
        self.frames = [big_frame(self.db, rot(2 * f), 70 + f) for f in range(3)]
        self.maps, self.t_maps = frames_world.maps, frames_world.t_maps      # the stages file's three depth / fill maps
        self.lists = []
        for (desc, uv), (img, fill) in zip(self.frames, self.maps):
            fr = synth.Frame(desc, uv, np.zeros(0, np.int32), np.zeros((0, 7), np.float32), np.zeros(0, np.int32), np.zeros(0, bool))
            self.lists.append(stages.oracle_lists(self.db, self.dbn, fr, img, fill))

    def context(self, reserve):
        c = capi.Context(0)
        c.db_upload(c.normalize(self.db.desc), self.db.model_of, self.db.xyz, self.db.n_models)
        c.reserve(reserve)
        c.frame_set_cluster_linkage(self.prm)
        return c

    def alone(self, c, f, seed=5):
        torch = self.torch
        m, fl = self.t_maps[f]
        c.frame_set_depth_image(m.data_ptr(), fl.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        desc, uv = self.frames[f]
        qd, tuv = torch.from_numpy(desc).to(self.dev), torch.from_numpy(uv).to(self.dev)
        c.frame_enqueue(qd.data_ptr(), tuv.data_ptr(), Q_BIG, K, CAM0, capi.default_frame_params(), seed + f)
        objs, counts = c.frame_fetch()
        return objs, counts, c.frame_fetch_matches_slot(0), stages.FrameWorld.table(c, 0), c.frame_counters()["error"]

    def step_table(self, c, f):
        """The frame's table from the step form, model by model, on the same context and depth map."""
        got = c.cluster_linkage([(uv, mx, wx) for _, uv, mx, wx in self.lists[f]], self.prm)
        return [(m, cl.tolist()) for m, (cls, _) in enumerate(got) if len(self.lists[f][m][0]) > self.prm.min_pts for cl in cls]


@pytest.fixture(scope="module")
def big(frames):
    return BigWorld(frames)


def test_big_frame_inputs(big):
    for f, ls in enumerate(big.lists):
        sizes = sorted(len(l[0]) for l in ls)
        print(f, sizes)
        assert sizes[0] == 0 and 1 <= sizes[1] <= 7 and 1 <= sizes[2] <= 7 and sizes[-2] > 160 and 1024 < sizes[-1] <= 1200


def test_frame_with_a_list_beyond_1024(big):
    w = big
    c = w.context(Q_BIG)
    try:
        with pytest.raises(capi.MhError, match="capacity exceeded .flags 1"):      # SCAN cuts the list at 1024 and says so
            w.alone(c, 0)
        assert c.frame_counters()["error"] & ERR_MS_CAP
        c.linkage_set_mode(ROWMAX)
        for rep in range(2):
            objs, counts, (mq, mm), table, err = w.alone(c, 0)
            assert err == 0, (rep, err)
            assert np.array_equal(mq, np.concatenate([l[0] for l in w.lists[0]]))
            want = w.step_table(c, 0)
            assert table == want and counts[1] == len(table), rep
            assert len(table) >= 3 and any(m == 0 for m, _ in table)        # (model 0: the list of 1200)
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()


def test_merged_batch_of_big_frames(big):
    w = big
    torch = w.torch
    c = w.context(3 * Q_BIG)
    try:
        c.linkage_set_mode(ROWMAX)
        alone = []
        for f in range(3):
            alone.append(w.alone(c, f))
            assert alone[f][4] == 0 and alone[f][3] == w.step_table(c, f), f      # (the step form over frame f's map)
        assert alone[0][3] != alone[1][3]
        c.frame_set_depth_image_batch([m.data_ptr() for m, _ in w.t_maps], [fl.data_ptr() for _, fl in w.t_maps], W, H,
                                      capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        uv = torch.cat([torch.from_numpy(u) for _, u in w.frames]).to(w.dev)
        for rep in range(2):
            qd = torch.cat([torch.from_numpy(d) for d, _ in w.frames]).to(w.dev)
            c.frame_enqueue_batch(qd.data_ptr(), uv.data_ptr(), Q_BIG, 3, K, CAM0, capi.default_frame_params(), [5, 6, 7])
            for f in range(3):
                objs, counts = c.frame_fetch_slot(f)
                a_objs, a_counts, (a_q, a_m), a_table, _ = alone[f]
                assert np.array_equal(counts, a_counts), (rep, f)
                mq, mm = c.frame_fetch_matches_slot(f)      # (every slot's lists are there: the batch stayed merged)
                assert np.array_equal(mq, a_q) and np.array_equal(mm, a_m), (rep, f)
                assert stages.FrameWorld.table(c, f) == a_table, (rep, f)
                assert objs.tobytes() == a_objs.tobytes(), (rep, f)
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()


# ---- 6: errors and state ---------------------------------------------------------------------------------------------------

def test_errors_and_state(device):
    c = device.c
    device.use("flat")
    assert c.linkage_get_mode() == SCAN
    with pytest.raises(capi.MhError, match="-> -1:"):
        c.linkage_set_mode(2)
    assert c.linkage_get_mode() == SCAN
    c.linkage_set_mode(ROWMAX)
    assert c.linkage_get_mode() == ROWMAX
    with pytest.raises(capi.MhError):
        c.linkage_set_mode(-1)
    assert c.linkage_get_mode() == ROWMAX
    try:
        c.linkage_stats(reset=True)
        big = np.zeros((capi.LINKAGE_MAX_POINTS + 1, 3), np.float32)
        with pytest.raises(capi.MhError, match="-> -3: .*more than 4096"):
            c.cluster_linkage([(big[:, :2], big, big)])
        with pytest.raises(capi.MhError, match="1 .. 4096"):
            c.linkage_debug_matrix(big[:, :2], big, big)
        with pytest.raises(capi.MhError, match="1 .. 4096"):
            c.linkage_debug_agglomerate(np.zeros((4097, 4097), np.float32))
        with pytest.raises(capi.MhError, match="1 .. 4096"):
            c.linkage_debug_agglomerate(np.zeros((0, 0), np.float32))
        assert c.linkage_stats() == (0, 0, 0, 0)              # nothing was launched
    finally:
        c.linkage_set_mode(SCAN)


def test_scratch_limit_refuses_before_any_launch(device):
    """3 x 2000^2 floats are 46 MiB: a 16 MiB limit refuses the call before any launch, and the next small call works."""
    maps = device.maps
    c = capi.Context(0)
    try:
        c.set_linkage_scratch_limit(16 << 20)
        c.linkage_set_mode(ROWMAX)
        m, f = device.t["scene"]
        c.frame_set_depth_image(m.data_ptr(), f.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        name, uv, mx, world = family_case("scene", 2000, maps)
        with pytest.raises(capi.MhError, match="MiB of similarity-matrix scratch"):
            c.cluster_linkage([(uv, mx, world)])
        assert c.linkage_stats() == (0, 0, 0, 0)
        name, uv, mx, world = family_case("scene", 45, maps)
        prm = capi.mh_linkage_params(0.3, 1, 2, -1.0, -1.0, 1)
        (clusters, _), = c.cluster_linkage([(uv, mx, world)], prm)
        _, Km = c.linkage_debug_matrix(uv, mx, world, prm)
        assert lists(clusters) == lists(orclib.linkage_agglomerate(Km, 0.3, 1, 1))
        assert c.linkage_stats()[0] == 2
    finally:
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()


def test_scan_rowmax_scan_on_one_context(device):
    c = device.c
    problems = []
    device.use("scene")
    for n in (5, 161, 64, 300):
        _, uv, mx, world = family_case("scene", n, device.maps)
        problems.append((uv, mx, world))
    prm = capi.mh_linkage_params(0.3, 1, 2, -1.0, -1.0, 1)
    out = []
    for mode in (SCAN, ROWMAX, SCAN, ROWMAX):
        c.linkage_set_mode(mode)
        out.append([(lists(cl), lab.tolist()) for cl, lab in c.cluster_linkage(problems, prm)])
    c.linkage_set_mode(SCAN)
    assert out[0] == out[1] == out[2] == out[3]
    assert sum(len(cl) for cl, _ in out[0]) >= 4


# ---- 7: hosts ------------------------------------------------------------------------------------------------------------------

def kinect_scene(path):
    """Scene B of tests/test_gpu_host_moped3d.py: bundled frame 0's keypoints on a plane are model 0, 500 clutter rows
    model 1, over the 640 x 480 "blobs" map, unfilled, fill_scale 8 -- a scene with an image, for the one-step plugin."""
    import dump_scene
    from test_gpu_depthfill import holes
    gray = np.ascontiguousarray(np.load(os.path.join(host3d.ROOT, "tests", "golden", "sift_ref_frames.npz"))["gray0"])
    c = capi.Context(0)
    try:
        xy, _, desc = c.sift(gray)
    finally:
        c.close()
    z = np.float32(0.8)
    xyz = np.stack([(xy[:, 0] - K[2]) / K[0] * z, (xy[:, 1] - K[3]) / K[1] * z, np.full(len(xy), z)], 1).astype(np.float32)
    rng = np.random.default_rng(7)
    db_desc = np.concatenate([desc, np.abs(rng.normal(size=(500, 128))).astype(np.float32)])
    db_xyz = np.concatenate([xyz, rng.uniform(-0.1, 0.1, (500, 3)).astype(np.float32)])
    model_of = np.concatenate([np.zeros(len(xy), np.int32), np.ones(500, np.int32)])
    zmap = np.full((H, W), 0.8, np.float32)
    zmap[holes("blobs", H, W, np.random.default_rng(3))[..., 2] < 0] = -1.0
    raw = np.zeros((H, W, 4), np.float32)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    raw[..., 2] = zmap
    raw[..., 0] = (u - K[2]) / K[0] * zmap
    raw[..., 1] = (v - K[3]) / K[1] * zmap
    raw[..., 3] = np.sqrt((raw[..., :3] ** 2).sum(-1))
    dump_scene.dump_kinect(path, db_desc, db_xyz, model_of, 2, raw, K, CAM0, gray=gray, patch_size=64, feature_density=0.8,
                           match_density=0.01, fill_scale=8, max_keypoints=1024)


def test_harness_with_linkage_rowmax(tmp_path):
    """moped3d_hip_test --linkage-rowmax (CLUSTER_LINKAGE_HIP's RowMaxima key; --resident: FRAME_RESIDENT_3D_HIP's
    LinkageRowMaxima) ends with the clusters and objects of the run without it, in the step wiring and the one step."""
    import dump_scene
    db = synth.make_db(4, 600)
    fr = synth.make_frame(db, n_vis=2, seed=5, Q=800)
    img, fill = synth.depth_image(db, fr, seed=5)
    path = str(tmp_path / "scene_a.bin")
    dump_scene.dump_kinect(path, db.desc, db.xyz, db.model_of, db.n_models, img, K, CAM0, uv=fr.uv, desc=fr.desc, distance=fill,
                           patch_size=64, feature_density=host3d.FEATURE_DENSITY, match_density=host3d.MATCH_DENSITY, fill_scale=0)
    plain, _ = host3d.run_harness([path])
    rowmax, _ = host3d.run_harness(["--linkage-rowmax", path])
    assert len(plain["CLUSTER"]["clusters"]) >= 2 and len(plain["FILTER2"]["objs"]) >= 2
    assert rowmax["CLUSTER"]["clusters"] == plain["CLUSTER"]["clusters"]
    assert rowmax["FILTER2"]["objs"] == plain["FILTER2"]["objs"]
    path_b = str(tmp_path / "scene_b.bin")
    kinect_scene(path_b)
    plain, extra = host3d.run_harness(["--resident", path_b])
    rowmax, extra_r = host3d.run_harness(["--resident", "--linkage-rowmax", path_b])
    assert len(plain["DEPTHFILL"]["objs"]) >= 1 and extra["counts"][1] >= 1
    assert rowmax["DEPTHFILL"]["objs"] == plain["DEPTHFILL"]["objs"] and extra_r["counts"] == extra["counts"]
    assert rowmax["DEPTHFILL"]["clusters"] == plain["DEPTHFILL"]["clusters"]
