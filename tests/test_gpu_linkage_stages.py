"""The linkage clusterer (moped_amd/csrc/linkage.hip; moped3d's CLUSTER_LINKAGE_CPU) stage by stage.

1. MATRIX.  mh_linkage_debug_matrix hands out A (the 3-D side after pass 2) and K (the similarity the agglomeration
   first sees).  Against the oracle's matrices (oracle/linkage_oracle.cpp, float32 with glibc's expf / atan2f) and a
   float64 restatement (tests/linkage_ref.py similarity_f64): equal NaN masks, K bit-symmetric, and with
       e_ref = max |K_oracle - K_f64|,  e_dev = max |K_device - K_f64|   (all non-NaN elements of the case, none left out)
   e_dev <= max(4 e_ref, 2^-21); the same for A with the floor scaled by A's maximum.  Device and oracle share every
   float32 rounding of the chain and differ in expf / atan2f only (OpenCL-profile bounds 3 and 6 ulp against glibc's <= 1);
   e_ref contains the chain's own roundings, including the ~25-fold amplification of an angle error by the discontinuity
   kernel near its steepest point.  The floor is 4 ulp at 1.0, for cases such as the flat lattice where e_ref is 0 and
   only an expf differs.
2. MERGE LOOP, exact.  (a) On the device's own matrix: mh_cluster_linkage's clusters, member order and labels equal
   orc_linkage_agglomerate(K_device) -- no tolerance, and an ulp of difference in K cannot fail it.  (b) On given matrices
   (mh_linkage_debug_agglomerate: the shipped loop over an uploaded matrix): ties, NaN, the last row pair, everything below
   the cutoff, minimum linkage's 1e20 rows, min_pts at the boundary.
3. FRAME FORM (linkage_models_kernel: what mh_frame_* run).  The cluster table of a slot
   (mh_frame_debug_fetch_clusters_slot) equals the oracle's per model and the batch form's, on a 20-model frame with more
   busy models than workgroups, one list beyond the LDS matrix's 160 rows, lists of 0 and <= min_pts matches; and every
   slot of a merged batch of three frames with their own depth and fill maps equals that frame alone.

Sizes: 1, 2, 3; 16 | 17 (the 16 wavefronts' row loop wraps); 44 | 45 (N (N + 1) / 2 crosses 1024 threads); 63, 64 | 65 and
128 | 129 (the lane stride along a row wraps); 159, 160 | 161 (LDS | global similarity matrix); 257; 1024 (LK_CAP) once.
Every family meets every size; the parameters rotate so that every value of each meets every size.

Largest errors per family (MI355X, all sizes and parameters of the table; every case prints its own):
    family            K: e_ref    e_dev        A: e_ref    e_dev
    scene                3.67e-07  3.67e-07       9.16e-07  9.16e-07
    lattice              3.45e-07  3.45e-07       1.03e-06  1.03e-06
    step                 4.47e-07  4.47e-07       1.18e-06  1.18e-06
    edges                4.21e-07  4.31e-07       7.31e-07  7.31e-07
    same_pixel           0         0              5.40e-29  5.40e-29
    same_model_point     3.44e-07  3.44e-07       1.02e-06  1.02e-06
    fill                 2.62e-07  2.62e-07       6.51e-07  6.51e-07
(same_pixel: with automatic sigmas every similarity is NaN, with fixed ones every K is exactly 1.)  On most cases the
device's matrices are the oracle's bit for bit; where they are not, e_dev stays within 1.3 e_ref."""
import numpy as np
import pytest

import linkage_ref as ref
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
W, H = 640, 480
SIZES = (1, 2, 3, 16, 17, 44, 45, 63, 64, 65, 128, 129, 159, 160, 161, 257)
FAMILIES = ("scene", "lattice", "step", "edges", "same_pixel", "same_model_point", "fill")
CUTOFFS = (0.05, 0.3, 0.6)
FLOOR = 2.0 ** -21


# ---- inputs ---------------------------------------------------------------------------------------------------------

def scene_map():
    """tests/test_gpu_linkage.py's depth map: planted object points in front of a wavy background, 5 % invalid pixels."""
    db = synth.make_db(6, 1500, seed=5)
    fr = synth.make_frame(db, n_vis=2, seed=21, Q=1600, pts_per_obj=140)
    return synth.depth_image(db, fr, seed=21, fill_max=0.3)


def make_maps():
    rng = np.random.default_rng(17)
    img, fill = scene_map()
    step = ref.flat_map(1.0)
    step[:, 320:, :] *= np.float32(1.5)
    big_fill = (rng.uniform(0, 60, (H, W)) * (rng.random((H, W)) < 0.5)).astype(np.float32)
    edges = img.copy()
    edges[60:100, :, 2] = np.nan                       # a band without depth
    return {"scene": (img, fill), "flat": (ref.flat_map(1.0), np.zeros((H, W), np.float32)), "step": (step, big_fill),
            "edges": (edges, big_fill)}


def family_case(family, n, maps):
    """-> (map name, uv, model points, world points) of `n` matches."""
    rng = np.random.default_rng([FAMILIES.index(family), n])
    noise = lambda w: (w + rng.normal(0, 0.002, w.shape)).astype(np.float32)
    if family == "scene":
        name, uv = "scene", rng.uniform([5, 5], [634, 474], (n, 2)).astype(np.float32)
    elif family == "lattice":
        name, uv = "flat", ref.lattice(n)
    elif family == "step":
        name = "step"
        a = rng.uniform([270, 200], [316, 246], ((n + 1) // 2, 2))
        b = rng.uniform([324, 200], [370, 246], (n // 2, 2))
        uv = np.concatenate([a, b]).astype(np.float32)
    elif family == "edges":
        name = "edges"
        img = maps[name][0]
        inv = np.argwhere(img[..., 3] < 0)
        uv = rng.uniform([0, 0], [W, H], (n, 2))
        k = np.arange(n)
        uv[k % 8 == 0, 1] = 0.3                         # border rows and columns, and points beyond them
        uv[k % 8 == 1, 1] = H - 0.5
        uv[k % 8 == 2, 0] = 0.7
        uv[k % 8 == 3, 0] = W + 1.5
        uv[k % 8 == 4, 1] = -2.25
        pick = inv[rng.integers(0, len(inv), n)]
        uv[k % 8 == 5] = pick[k % 8 == 5][:, ::-1] + 0.5  # invalid pixels (norm < 0)
        uv[k % 8 == 6, 1] = rng.uniform(60, 100, int((k % 8 == 6).sum()))   # the band of NaN depths
        uv = uv.astype(np.float32)
    elif family == "same_pixel":
        name, uv = "scene", np.repeat(np.array([[310.2, 221.7]], np.float32), n, 0)
    elif family == "same_model_point":
        name, uv = "step", rng.uniform([200, 150], [440, 330], (n, 2)).astype(np.float32)
    elif family == "fill":
        name, uv = "step", rng.uniform([5, 5], [634, 474], (n, 2)).astype(np.float32)
    world = ref.world_of(maps[name][0], uv)
    mx = noise(world)
    if family == "same_pixel":
        mx = (world + rng.normal(0, 0.02, world.shape)).astype(np.float32)
    if family == "same_model_point":
        mx[: (n + 1) // 2] = mx[0]                      # K3F divides by a zero model distance there
    return name, uv, mx, world


def case_params(family, n):
    """The parameters of (family, size): rotated so that every value of each parameter meets every size."""
    f, s = FAMILIES.index(family), SIZES.index(n) if n in SIZES else 0
    use3d = (f + s) % 3
    sig = (-1.0, -1.0) if (f + s) % 2 == 0 else (14.0, 0.03)
    ltype = (f + f // 3 + 2 * s) % 3
    cutoff = CUTOFFS[(2 * f + s) % 3]
    min_pts = (0, 1, 3)[(f + s) % 3]
    return use3d, sig, ltype, cutoff, min_pts


class Device:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.c = capi.Context(0)
        self.maps = make_maps()
        self.t = {k: (torch.from_numpy(m).to(self.dev), torch.from_numpy(f).to(self.dev)) for k, (m, f) in self.maps.items()}
        torch.cuda.synchronize()
        self.current = None

    def use(self, name):
        if self.current != name:
            m, f = self.t[name]
            self.c.frame_set_depth_image(m.data_ptr(), f.data_ptr(), W, H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
            self.current = name

    def close(self):
        self.c.frame_set_depth_image(0, 0, 0, 0, 0)
        self.c.close()


@pytest.fixture(scope="module")
def device():
    d = Device()
    yield d
    d.close()


def _labels(n, clusters):
    lab = np.full(n, -1, np.int32)
    for k, cl in enumerate(clusters):
        lab[cl] = k
    return lab


def _same(got, want, tag):
    assert [c.tolist() for c in got] == [c.tolist() for c in want], tag     # same members in the same (reference) order


# ---- 1 + 2a: the matrix against oracle and float64, the merge loop on the device's own matrix -----------------------------

def check_case(device, family, n, linkage_type=None):
    name, uv, mx, world = family_case(family, n, device.maps)
    use3d, sig, ltype, cutoff, min_pts = case_params(family, n)
    if linkage_type is not None:
        ltype = linkage_type
    tag = (family, n, use3d, sig, ltype, cutoff, min_pts)
    img, fill = device.maps[name]
    device.use(name)
    prm = capi.mh_linkage_params(cutoff, min_pts, use3d, sig[0], sig[1], ltype)
    A_dev, K_dev = device.c.linkage_debug_matrix(uv, mx, world, prm)
    _, K_orc, A_orc = orclib.cluster_linkage(uv, mx, world, img, fill, use3d_filter=use3d, sigma2d=sig[0], sigma3d=sig[1],
                                             want_k=True, want_a=True)
    A64, K64 = ref.similarity_f64(uv, mx, world, img, fill, use3d, *sig)
    for what, dev_m, orc_m, f64_m in (("K", K_dev, K_orc, K64), ("A", A_dev, A_orc, A64)):
        nan = np.isnan(orc_m)
        assert np.array_equal(np.isnan(dev_m), nan), (tag, what, "NaN mask")
        assert np.array_equal(np.isnan(f64_m), nan), (tag, what, "NaN mask of the float64 restatement")
        assert np.array_equal(dev_m.view(np.uint32), dev_m.T.view(np.uint32)), (tag, what, "not symmetric bit for bit")
        ok = ~nan
        e_ref = float(np.abs(orc_m[ok].astype(np.float64) - f64_m[ok]).max()) if ok.any() else 0.0
        e_dev = float(np.abs(dev_m[ok].astype(np.float64) - f64_m[ok]).max()) if ok.any() else 0.0
        scale = 1.0 if what == "K" else (float(np.abs(f64_m[ok]).max()) if ok.any() else 1.0)
        print(tag, what, "e_ref %.3g e_dev %.3g floor %.3g" % (e_ref, e_dev, FLOOR * scale))
        assert e_dev <= max(4 * e_ref, FLOOR * scale), (tag, what, e_ref, e_dev)
    # the merge loop, exact, from the device's own matrix
    (clusters, label), = device.c.cluster_linkage([(uv, mx, world)], prm)
    want = orclib.linkage_agglomerate(K_dev, cutoff, min_pts, ltype)
    _same(clusters, want, tag)
    assert np.array_equal(label, _labels(n, want)), tag


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_matrix_and_merge_loop(device, family, n):
    check_case(device, family, n)


def test_lk_cap_rows_average_linkage(device):
    """N = 1024 = LK_CAP: one row element per thread, the similarity matrix in global memory."""
    check_case(device, "scene", 1024, linkage_type=1)


def test_case_table_covers_parameters_and_cluster_counts():
    """CPU side: every value of every parameter meets every size, and over the oracle's own matrices the table's cutoffs
    give no, one, several and many clusters -- the merge-loop cases above are not all trivial."""
    maps = make_maps()
    counts = []
    for n in SIZES:
        seen = [set() for _ in range(5)]
        for family in FAMILIES:
            prm = case_params(family, n)
            for k, v in enumerate(prm):
                seen[k].add(v)
            name, uv, mx, world = family_case(family, n, maps)
            use3d, sig, ltype, cutoff, min_pts = prm
            if n >= 16:
                counts.append(len(orclib.cluster_linkage(uv, mx, world, *maps[name], cutoff=cutoff, min_pts=min_pts,
                                                         use3d_filter=use3d, linkage_type=ltype, sigma2d=sig[0],
                                                         sigma3d=sig[1])))
        assert [len(x) for x in seen] == [3, 2, 3, 3, 3], (n, seen)
    print(sorted(counts))
    assert 0 in counts and 1 in counts and any(2 <= k <= 5 for k in counts) and any(k > 5 for k in counts)


# ---- 2b: the merge loop on given matrices ----------------------------------------------------------------------------------

def three_valued(n, seed, rng=None):
    rng = np.random.default_rng([n, seed])
    M = rng.choice(np.array([0.2, 0.5, 0.8], np.float32), (n, n))
    return np.ascontiguousarray(np.triu(M) + np.triu(M, 1).T, np.float32)


def given_matrices(n):
    rng = np.random.default_rng(n)
    flat = ref.flat_map()
    uv = ref.lattice(n)
    w = ref.world_of(flat, uv)
    _, lat = orclib.cluster_linkage(uv, w, w, flat, None, min_pts=0, want_k=True)
    out = {"lattice": lat, "three_valued": three_valued(n, 1), "all_equal": np.full((n, n), 0.5, np.float32)}
    last = rng.uniform(0.1, 0.4, (n, n)).astype(np.float32)
    last = np.triu(last) + np.triu(last, 1).T
    last[n - 2, n - 1] = last[n - 1, n - 2] = 0.9
    out["last_row_pair"] = last
    holes = three_valued(n, 2)
    hole = np.triu(rng.random((n, n)) < 0.3, 1)
    holes[hole | hole.T] = np.nan
    holes[0, :] = holes[:, 0] = np.nan
    out["nan_entries"] = holes
    out["below_cutoff"] = (three_valued(n, 3) * np.float32(0.1)).astype(np.float32)
    return out


@pytest.mark.parametrize("n", (2, 3, 17, 64, 65, 160, 161, 257))
def test_merge_loop_on_given_matrices(device, n):
    c = device.c
    merged = 0
    for name, M in given_matrices(n).items():
        for ltype in (0, 1, 2):
            for cutoff in (0.3, 0.6):
                tag = (n, name, ltype, cutoff)
                clusters, label = c.linkage_debug_agglomerate(M, cutoff, 0, ltype)
                want = orclib.linkage_agglomerate(M, cutoff, 0, ltype)
                _same(clusters, want, tag)
                assert np.array_equal(label, _labels(n, want)), tag
                merged += len(want) < n
                if name == "below_cutoff":
                    assert len(want) == n, tag
                if name == "last_row_pair" and cutoff == 0.6:
                    assert [cl.tolist() for cl in want if len(cl) > 1] == [[n - 2, n - 1]], tag
                if name == "all_equal" and cutoff == 0.3 and ltype != 0:
                    assert want[0][:2].tolist() == [0, 1], tag            # the first pair wins the first scan
    assert merged >= 20


def test_minimum_linkage_reaches_an_emptied_clusters_row(device):
    """Minimum linkage gives the row of a merged cluster 1e20 where the other cluster is empty (minimumLinkage over
    nothing), and the absorbed index is still listed in the next scan: that 1e20 wins it, a merge with an empty cluster.
    The witness counts those merges, so the input is known to get there; device = oracle = witness."""
    for n, M in ((17, np.full((17, 17), 0.5, np.float32)), (36, given_matrices(36)["lattice"])):
        want, stats = ref.agglomerate(M, 0.3, 0, 0)
        assert stats["stale"] >= n // 2 - 1, stats
        clusters, _ = device.c.linkage_debug_agglomerate(M, 0.3, 0, 0)
        assert [cl.tolist() for cl in clusters] == want
        assert [cl.tolist() for cl in orclib.linkage_agglomerate(M, 0.3, 0, 0)] == want


def test_min_pts_counts_strictly(device):
    """A cluster is emitted with MORE than min_pts members (:535): sizes 4 and 3 at min_pts 2, 3 and 4."""
    M = np.full((7, 7), 0.1, np.float32)
    M[:4, :4] = 0.9
    M[4:, 4:] = 0.9
    for ltype in (0, 1, 2):
        for min_pts, sizes in ((2, [4, 3]), (3, [4]), (4, [])):
            clusters, label = device.c.linkage_debug_agglomerate(M, 0.5, min_pts, ltype)
            want = orclib.linkage_agglomerate(M, 0.5, min_pts, ltype)
            _same(clusters, want, (ltype, min_pts))
            assert [len(cl) for cl in clusters] == sizes and np.array_equal(label, _labels(7, want))


def test_debug_exports_refuse_wrong_sizes(device):
    c = device.c
    device.use("flat")
    z2, z3 = np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32)
    with pytest.raises(capi.MhError, match="1 .. 1024"):
        c.linkage_debug_matrix(z2, z3, z3)
    big = np.zeros((1025, 3), np.float32)
    with pytest.raises(capi.MhError, match="1 .. 1024"):
        c.linkage_debug_matrix(big[:, :2], big, big)
    with pytest.raises(capi.MhError, match="1 .. 1024"):
        c.linkage_debug_agglomerate(np.zeros((1025, 1025), np.float32))
    with pytest.raises(capi.MhError, match="1 .. 1024"):
        c.linkage_debug_agglomerate(np.zeros((0, 0), np.float32))
    with pytest.raises(capi.MhError, match="linkage_type"):
        c.linkage_debug_agglomerate(np.zeros((3, 3), np.float32), linkage_type=3)
    c.frame_set_depth_image(0, 0, 0, 0, 0)
    device.current = None
    one = np.zeros((1, 3), np.float32)
    with pytest.raises(capi.MhError, match="no depth map"):
        c.linkage_debug_matrix(one[:, :2], one, one)
    # (the agglomeration needs none)
    clusters, _ = c.linkage_debug_agglomerate(np.full((3, 3), 0.5, np.float32), 0.3, 0, 1)
    assert [cl.tolist() for cl in clusters] == [cl.tolist() for cl in orclib.linkage_agglomerate(np.full((3, 3), 0.5, np.float32), 0.3, 0, 1)]


# ---- 3: the frame form ---------------------------------------------------------------------------------------------------------

N_MODELS, Q_FRAME = 20, 1024
# planted matches per model: one list beyond the LDS matrix (200), two models without any, three with 1 .. min_pts
PLANTED = (30, 0, 12, 200, 5, 45, 9, 64, 0, 17, 7, 100, 65, 20, 16, 33, 129, 10, 3, 50)


def counted_frame(db, planted, seed):
    """A frame with planted[m] features of model m (synth.make_frame's recipe with a count per model) and clutter that
    matches nothing (random directions: no nearest neighbour stands out)."""
    rng = np.random.default_rng([0xC1, seed])
    descs, uvs, srcs, outl, poses, visible = [], [], [], [], [], []
    for m, k in enumerate(planted):
        if k == 0:
            continue
        rows = np.nonzero(db.model_of == m)[0]
        while True:
            z = rng.uniform(0.6, 1.0)
            u0, v0 = rng.uniform(120, W - 120), rng.uniform(100, H - 100)
            pose = np.concatenate([synth.random_quat(rng), [(u0 - K[2]) / K[0] * z, (v0 - K[3]) / K[1] * z, z]]).astype(np.float32)
            uv_all, zc = synth.project_np(pose, db.xyz[rows], K)
            ok = (zc > 0.05) & (uv_all[:, 0] >= 0) & (uv_all[:, 0] < W) & (uv_all[:, 1] >= 0) & (uv_all[:, 1] < H)
            if ok.sum() >= k:
                break
        sel = rng.choice(np.nonzero(ok)[0], size=k, replace=False)
        uv = uv_all[sel] + rng.uniform(-0.5, 0.5, (k, 2))
        bad = rng.random(k) < 0.15
        uv[bad] = rng.uniform([0, 0], [W, H], (int(bad.sum()), 2))
        d = db.desc[rows[sel]] + rng.normal(0, 0.01, (k, 128)).astype(np.float32)
        descs.append(synth.l2_normalize(np.maximum(d, 0).astype(np.float32)))
        uvs.append(uv.astype(np.float32))
        srcs.append(rows[sel].astype(np.int32))
        outl.append(bad)
        poses.append(pose)
        visible.append(m)
    n_clutter = Q_FRAME - sum(planted)
    descs.append(synth.l2_normalize(np.abs(rng.normal(size=(n_clutter, 128))).astype(np.float32)))
    uvs.append(rng.uniform([0, 0], [W, H], (n_clutter, 2)).astype(np.float32))
    srcs.append(np.full(n_clutter, -1, np.int32))
    outl.append(np.zeros(n_clutter, bool))
    perm = rng.permutation(Q_FRAME)
    return synth.Frame(np.ascontiguousarray(np.concatenate(descs)[perm]), np.ascontiguousarray(np.concatenate(uvs)[perm]),
                       np.array(visible, np.int32), np.array(poses, np.float32), np.concatenate(srcs)[perm],
                       np.concatenate(outl)[perm])


def frame_maps(db, fr, f):
    """Frame f's depth and fill maps: the planted points over the wavy background, depth steps along bands whose place
    and width depend on f, fill distances that matter (up to 50 px against gamma = 25) from a pattern of its own."""
    rng = np.random.default_rng([0xF1, f])
    img, _ = synth.depth_image(db, fr, seed=f, fill_max=0.3)
    u = np.arange(W)
    far = ((u + 37 * f) // (60 + 15 * f)) % 2 == 1
    img[:, far, :3] *= np.float32(1.25)
    img[..., 3] = np.where(img[..., 3] < 0, -1.0, np.sqrt((img[..., :3] ** 2).sum(-1)))
    fill = (rng.uniform(0, 50, (H, W)) * (rng.random((H, W)) < 0.5)).astype(np.float32)
    return np.ascontiguousarray(img, np.float32), fill


def oracle_lists(db, dbn, fr, img, fill):
    """-> per model (queries, uv, model points, world points) of the oracle's match lists."""
    idx, d1, d2 = orclib.match_2nn(dbn, orclib.normalize(fr.desc))
    out_q, off = orclib.match_accept(idx, d1, d2, 0.8, db.model_of, db.n_models)
    lists = []
    for m in range(db.n_models):
        q = out_q[off[m]:off[m + 1]]
        uv = fr.uv[q]
        world, _ = orclib.depthmap_prop(img, fill, uv, 0.1)
        lists.append((q, uv, db.xyz[idx[q]], world))
    return lists


def oracle_table(lists, img, fill, prm):
    """The frame's cluster table: (model, members in order) in (model, emission) order; models without work skipped."""
    table = []
    for m, (q, uv, mx, world) in enumerate(lists):
        if len(q) <= prm.min_pts:
            continue
        for cl in orclib.cluster_linkage(uv, mx, world, img, fill, cutoff=prm.cutoff, min_pts=prm.min_pts,
                                         use3d_filter=prm.use3d_filter, linkage_type=prm.linkage_type):
            table.append((m, cl.tolist()))
    return table


class FrameWorld:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.db = synth.make_db(N_MODELS, 400, seed=11)
        self.dbn = orclib.normalize(self.db.desc)
        self.prm = capi.default_linkage_params()
        rot = lambda k: PLANTED[k:] + PLANTED[:k]
        self.frames = [counted_frame(self.db, rot(7 * f), 40 + f) for f in range(3)]
        self.maps = [frame_maps(self.db, fr, f) for f, fr in enumerate(self.frames)]
        self.lists = [oracle_lists(self.db, self.dbn, fr, *mp) for fr, mp in zip(self.frames, self.maps)]
        self.tables = [oracle_table(ls, *mp, self.prm) for ls, mp in zip(self.lists, self.maps)]
        self.t_maps = [(torch.from_numpy(m).to(self.dev), torch.from_numpy(f).to(self.dev)) for m, f in self.maps]
        torch.cuda.synchronize()

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
        fr = self.frames[f]
        qd, uv = torch.from_numpy(fr.desc).to(self.dev), torch.from_numpy(fr.uv).to(self.dev)
        c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), Q_FRAME, K, CAM0, capi.default_frame_params(), seed + f)
        objs, counts = c.frame_fetch()
        return objs, counts, c.frame_fetch_matches_slot(0), self.table(c, 0)

    @staticmethod
    def table(c, slot):
        return [(m, mem.tolist()) for m, mem in c.frame_debug_fetch_clusters_slot(slot)]


@pytest.fixture(scope="module")
def frames():
    return FrameWorld()


def test_frame_inputs_bite(frames):
    """CPU side, before the device is trusted: the frames have what the frame form is to be tested with, and every
    frame's table changes when it is computed over another frame's maps."""
    w = frames
    for f, lists in enumerate(w.lists):
        sizes = np.array([len(l[0]) for l in lists])
        print(f, sizes.tolist(), len(w.tables[f]))
        assert (sizes > w.prm.min_pts).sum() >= 12 and (sizes > 160).sum() == 1
        assert ((sizes >= 1) & (sizes <= w.prm.min_pts)).sum() >= 2 and (sizes == 0).sum() >= 2
        assert len(w.tables[f]) >= 12 and len({m for m, _ in w.tables[f]}) >= 10
        assert max(len(cl) for _, cl in w.tables[f]) >= 20
    # more models with work than the first CLUSTER launch of a context has workgroups (frame_rest.hip: 8)
    assert (np.array([len(l[0]) for l in w.lists[0]]) > w.prm.min_pts).sum() > 8
    for f in range(3):
        for g in range(3):
            if g != f:      # frame f's lists over frame g's maps: what a kernel that read the wrong slot's maps would give
                assert oracle_table(w.lists[f], *w.maps[g], w.prm) != w.tables[f], (f, g)


def test_frame_form_cluster_table(frames):
    """One frame on a fresh context (its first CLUSTER launch: 8 workgroups for 15 models with work, so workgroups take a
    second model after a larger one): match lists, cluster table, batch form."""
    w = frames
    c = w.context(Q_FRAME)
    try:
        objs, counts, (mq, mm), table = w.alone(c, 0)
        lists = w.lists[0]
        assert np.array_equal(mq, np.concatenate([l[0] for l in lists]))
        assert np.array_equal(mm, np.concatenate([np.full(len(l[0]), m, np.int32) for m, l in enumerate(lists)]))
        assert table == w.tables[0]
        assert counts[0] == len(mq) and counts[1] == len(table)
        # the batch form (mh_cluster_linkage) on the same lists
        got = c.cluster_linkage([(uv, mx, wx) for _, uv, mx, wx in lists], w.prm)
        flat = [(m, cl.tolist()) for m, (cls, _) in enumerate(got) for cl in cls]
        assert flat == table
        assert len(objs) >= 1
        # and again on the same context (the launch is sized by what the first one found)
        assert w.alone(c, 0)[3] == table
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()


def test_merged_batch_slots_equal_frames_alone(frames):
    """Three frames with their own depth and fill maps in one merged batch (mh_frame_enqueue_batch over
    mh_frame_set_depth_image_batch): every slot's lists and cluster table are that frame's alone and the oracle's."""
    w = frames
    torch = w.torch
    c = w.context(3 * Q_FRAME)
    try:
        alone = [w.alone(c, f) for f in range(3)]
        for f in range(3):
            assert alone[f][3] == w.tables[f], f
        c.frame_set_depth_image_batch([m.data_ptr() for m, _ in w.t_maps], [fl.data_ptr() for _, fl in w.t_maps], W, H,
                                      capi.DEPTH_BACKPROJECTION, 0.5, 0.1)
        uv = torch.cat([torch.from_numpy(fr.uv) for fr in w.frames]).to(w.dev)
        for rep in range(2):
            qd = torch.cat([torch.from_numpy(fr.desc) for fr in w.frames]).to(w.dev)
            c.frame_enqueue_batch(qd.data_ptr(), uv.data_ptr(), Q_FRAME, 3, K, CAM0, capi.default_frame_params(), [5, 6, 7])
            for f in range(3):
                objs, counts = c.frame_fetch_slot(f)
                a_objs, a_counts, (a_q, a_m), a_table = alone[f]
                assert np.array_equal(counts, a_counts), (rep, f)
                mq, mm = c.frame_fetch_matches_slot(f)      # (every slot's lists are there: the batch stayed merged)
                assert np.array_equal(mq, a_q) and np.array_equal(mm, a_m), (rep, f)
                assert w.table(c, f) == a_table, (rep, f)
                assert objs.tobytes() == a_objs.tobytes(), (rep, f)
    finally:
        c.frame_set_cluster_linkage(None)
        c.frame_set_depth_image(0, 0, 0, 0, 0)
        c.close()
