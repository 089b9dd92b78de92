"""mh_object_hulls (csrc/hull.hip: Object::getObjectHull on the device) against tests/hull_ref.py -- the float32
restatement of getConvexHull that tests/test_hull_cpu.py holds to the reference's recorded outputs -- over the oracle's
project(): vertex values and vertex order equal, in both device forms (0: octagon prefilter, 1: everything sorted and
chained).  Models of 0, 1, 2, 3 rows, at the wavefront edge (63 / 64 / 65), at the workgroup edge (1 024 / 1 025) and of
5 000 rows; lattices full of ties, all-equal and collinear clouds, a plane seen edge-on; rings with
MH_HULL_LDS_POINTS and MH_HULL_LDS_POINTS + 1 points that the prefilter cannot thin (the second takes the global path);
n_behind; the vertex cap; the bounding-box corners; a database edit; the refusals."""
import ctypes as C

import numpy as np
import pytest

import hull_ref
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu

K = np.array([525.0, 525.0, 320.0, 240.0], np.float32)
K_UNIT = np.array([1.0, 1.0, 0.0, 0.0], np.float32)     # with IDENT and z = 1: (u, v) = (x, y) exactly
CAM = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
CAP = capi.HULL_LDS_POINTS
BOX_ROWS = [0, 1, 2, 3, 63, 64, 65, 1024, 1025, 5000]


def _ring(n, radius, rng):
    a = np.sort(rng.uniform(0, 2 * np.pi, n))
    return rng.permutation(np.stack([radius * np.cos(a), radius * np.sin(a), np.ones(n)], 1)).astype(np.float32)


def _models():
    """name -> xyz [n, 3]; the order is the model index."""
    rng = np.random.default_rng(0x4011D)
    m = {}
    for n in BOX_ROWS:
        m[f"box{n}"] = (rng.uniform(-0.5, 0.5, (n, 3)) * [0.3, 0.2, 0.1]).astype(np.float32)
    for n in (64, 65, 1025):
        side = 6 if n < 100 else 20
        m[f"lattice{n}"] = np.concatenate([rng.integers(-side, side + 1, (n, 2)), np.ones((n, 1))], 1).astype(np.float32)
        m[f"equal{n}"] = np.tile(np.array([[3.0, -2.0, 1.0]], np.float32), (n, 1))
        t = rng.integers(-30, 31, n).astype(np.float32)
        m[f"collinear{n}"] = np.stack([t, 2 * t + 1, np.ones(n, np.float32)], 1)
        m[f"plane{n}"] = np.concatenate([rng.uniform(-0.2, 0.2, (n, 2)), np.zeros((n, 1))], 1).astype(np.float32)
    m["ring200"] = _ring(200, 150.0, rng)
    m["ringcap"] = _ring(CAP, 200.0, rng)
    m["ringcap1"] = _ring(CAP + 1, 200.0, rng)
    return m


@pytest.fixture(scope="module")
def models():
    return _models()


def _upload(c, models):
    rng = np.random.default_rng(7)
    xyz = np.concatenate(list(models.values())).astype(np.float32)
    model_of = np.concatenate([np.full(len(v), i, np.int32) for i, v in enumerate(models.values())])
    desc = synth.l2_normalize(rng.normal(size=(len(xyz), 128)).astype(np.float32))
    c.db_upload(desc, model_of, xyz, len(models))
    return desc, model_of, xyz


@pytest.fixture(scope="module")
def hctx(models):
    """A context of this module's own (the session's carries other tests' databases)."""
    c = capi.Context(0)
    _upload(c, models)
    yield c
    c.close()


def _pose(rng, z=(0.6, 1.4)):
    return np.concatenate([synth.random_quat(rng), [rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(*z)]]).astype(np.float32)


def _edge_on(rng, tilt):
    """The model's z = 0 plane turned about x by 90 degrees minus `tilt`, through the camera centre (t_y = 0): seen
    edge-on (tilt 0: every v within rounding of c_y) or as a thin sliver."""
    a = np.pi / 2 - tilt
    return np.array([np.sin(a / 2), 0, 0, np.cos(a / 2), rng.uniform(-0.1, 0.1), 0.0, 0.8], np.float32)


def _objects(models):
    """(model index, pose, K) of every object the forms are compared on."""
    rng = np.random.default_rng(0x0B1)
    names = list(models)
    objs = []
    for i, name in enumerate(names):
        if name.startswith("box"):
            objs += [(i, _pose(rng), K) for _ in range(3)]
        elif name.startswith("plane"):
            objs += [(i, _edge_on(rng, t), K) for t in (0.0, 1e-6, 1e-4, 1e-2)] + [(i, _pose(rng), K)]
        else:
            objs += [(i, IDENT, K_UNIT), (i, _pose(rng, (40.0, 80.0)) if name.startswith("ring") else _pose(rng, (3.0, 6.0)), K)]
    return objs


def _same(got, want, what):
    assert hull_ref.same_vertices(got, want), (what, len(got), len(want))


@pytest.mark.parametrize("form", [0, 1])
def test_hulls_equal_the_restatement(hctx, models, form):
    names = list(models)
    xyzs = list(models.values())
    objs = _objects(models)
    hctx.hull_debug_form(form)
    try:
        seen = dict(empty=0, two=0, big=0)
        for Kc in (K, K_UNIT):
            sel = [o for o in objs if o[2] is Kc]
            hulls, nv, nb, bb = hctx.object_hulls([o[0] for o in sel], [o[1] for o in sel], Kc, CAM, max_vertices=2 * CAP + 8)
            for j, (m, pose, _) in enumerate(sel):
                want, behind = hull_ref.object_hull(pose, xyzs[m], Kc, CAM)
                what = (form, names[m], j)
                print(what, "vertices", nv[j], "want", len(want), "behind", nb[j])
                assert nv[j] == len(want) and nb[j] == behind, what
                _same(hulls[j], want, what)
                assert np.array_equal(bb[j], hull_ref.bbox_corners(pose, xyzs[m], Kc, CAM)), what
                seen["empty"] += len(want) == 0
                seen["two"] += len(want) == 2
                seen["big"] += len(want) > 1000
        assert seen["empty"] >= 2 and seen["two"] >= 6 and seen["big"] >= 2, seen
    finally:
        hctx.hull_debug_form(0)


def test_ring_models_are_not_thinned_by_the_prefilter(models):
    """What sends `ringcap1` down the global path in form 0: every point of a ring survives the prefilter."""
    for name in ("ringcap", "ringcap1"):
        uv, _ = hull_ref.project_front(IDENT, models[name], K_UNIT, CAM)
        assert len(hull_ref.prefilter(uv)) == len(models[name])


@pytest.mark.parametrize("form", [0, 1])
def test_points_behind_the_camera_are_counted_and_left_out(hctx, models, form):
    names = list(models)
    m = names.index("box5000")
    rng = np.random.default_rng(5)
    part = np.concatenate([synth.random_quat(rng), [0.0, 0.0, 0.01]]).astype(np.float32)     # the box straddles z = 0.001
    allb = np.concatenate([synth.random_quat(rng), [0.0, 0.0, -1.0]]).astype(np.float32)
    hctx.hull_debug_form(form)
    try:
        hulls, nv, nb, bb = hctx.object_hulls([m, m], [part, allb], K, CAM, max_vertices=256)
    finally:
        hctx.hull_debug_form(0)
    want, behind = hull_ref.object_hull(part, models["box5000"], K, CAM)
    assert 500 < behind < 4500 and nb[0] == behind and nv[0] == len(want) > 2
    _same(hulls[0], want, "part")
    assert nb[1] == 5000 and nv[1] == 0 and len(hulls[1]) == 0
    assert np.array_equal(bb[1], np.full((8, 2), hull_ref.FLT_MAX))      # project() of a corner behind the camera
    assert np.array_equal(bb[0], hull_ref.bbox_corners(part, models["box5000"], K, CAM))


def test_vertex_cap_reports_the_true_count_and_writes_the_first(hctx, models):
    m = list(models).index("ring200")
    want, _ = hull_ref.object_hull(IDENT, models["ring200"], K_UNIT, CAM)
    assert len(want) > 150
    xy = np.full((1, 64 + 3, 2), -7.0, np.float32)      # 64 rows for the call, a sentinel behind them
    nv = np.zeros(1, np.int32)
    c = capi.make_cam(K_UNIT, CAM)
    mod = np.array([m], np.int32)
    rc = hctx.L.mh_object_hulls(hctx.h, capi._ptr(mod), capi._ptr(IDENT), 1, C.byref(c), 64, capi._ptr(xy), capi._ptr(nv), None, None)
    assert rc == capi.MH_OK
    assert nv[0] == len(want)
    assert np.array_equal(xy[0, :64], want[:64])
    assert np.all(xy[0, 64:] == -7.0)


def test_hull_follows_a_database_edit(models):
    c = capi.Context(0)
    try:
        small = {k: models[k] for k in ("box64", "box1025", "lattice65")}
        _upload(c, small)
        rng = np.random.default_rng(11)
        pose = _pose(rng)
        before = c.object_hulls([1, 2], [pose, pose], K, CAM, 128)
        new_xyz = (rng.uniform(-0.5, 0.5, (333, 3)) * [0.1, 0.4, 0.2]).astype(np.float32)
        new_desc = synth.l2_normalize(rng.normal(size=(333, 128)).astype(np.float32))
        c.db_splice(capi.DB_REPLACE, 1, new_desc, new_xyz)
        after = c.object_hulls([1, 2], [pose, pose], K, CAM, 128)
        want, _ = hull_ref.object_hull(pose, new_xyz, K, CAM)
        _same(after[0][0], want, "replaced")
        assert not hull_ref.same_vertices(after[0][0], before[0][0])
        _same(after[0][1], before[0][1], "the model behind it moved with its rows")
        assert np.array_equal(after[3][0], hull_ref.bbox_corners(pose, new_xyz, K, CAM))
        c.db_splice(capi.DB_REMOVE, 0)                 # lattice65 is model 1 now
        moved = c.object_hulls([1], [pose], K, CAM, 128)
        _same(moved[0][0], before[0][1], "after a removal")
    finally:
        c.close()


def test_refusals_launch_nothing(hctx, models):
    L, h = hctx.L, hctx.h
    m = list(models).index("box65")
    rng = np.random.default_rng(3)
    pose = _pose(rng)
    good = hctx.object_hulls([m], [pose], K, CAM, 32)
    cam = capi.make_cam(K, CAM)
    mod = np.array([m], np.int32)

    def call(mod=mod, pose=pose, n=1, cam=cam, maxv=32, xy=True, nv=True):
        out_xy = np.full((1, 32, 2), -7.0, np.float32)
        out_nv = np.full(1, -7, np.int32)
        rc = L.mh_object_hulls(h, capi._ptr(mod), capi._ptr(pose), n, C.byref(cam) if cam is not None else None, maxv,
                               capi._ptr(out_xy) if xy else None, capi._ptr(out_nv) if nv else None, None, None)
        assert np.all(out_xy == -7.0) and out_nv[0] == -7     # nothing came back
        return rc

    bad_pose = pose.copy()
    bad_pose[5] = np.nan
    inf_pose = pose.copy()
    inf_pose[0] = np.inf
    for kw in (dict(mod=None), dict(pose=None), dict(cam=None), dict(xy=False), dict(nv=False), dict(maxv=0), dict(maxv=-1),
               dict(n=-1), dict(mod=np.array([len(models)], np.int32)), dict(mod=np.array([-1], np.int32)),
               dict(pose=bad_pose), dict(pose=inf_pose)):
        assert call(**kw) == capi.MH_ERR_ARG, kw
        assert L.mh_last_error(h).decode().startswith("mh_object_hulls"), kw
    assert call(n=0) == capi.MH_OK
    assert L.mh_hull_debug_form(h, 2) == capi.MH_ERR_ARG
    again = hctx.object_hulls([m], [pose], K, CAM, 32)      # the context is as it was
    _same(again[0][0], good[0][0], "after the refusals")

    # stores without whole models in ascending order: not grouped, uploaded in blocks
    c = capi.Context(0)
    try:
        desc = synth.l2_normalize(rng.normal(size=(256, 128)).astype(np.float32))
        xyz = rng.uniform(-0.1, 0.1, (256, 3)).astype(np.float32)
        c.db_upload(desc, np.array([1] * 128 + [0] * 128, np.int32), xyz, 2)
        with pytest.raises(capi.MhError, match="not grouped"):
            c.object_hulls([0], [pose], K, CAM, 32)
        c.db_upload_blocks(desc, np.array([0] * 128 + [1] * 128, np.int32), xyz, 2, [0, 512], [128, 128])
        with pytest.raises(capi.MhError, match="blocks"):
            c.object_hulls([0], [pose], K, CAM, 32)
        c.db_upload(desc, np.array([0] * 128 + [1] * 128, np.int32), xyz, 2)
        hulls, nv, nb, bb = c.object_hulls([1], [pose], K, CAM, 32)
        _same(hulls[0], hull_ref.object_hull(pose, xyz[128:], K, CAM)[0], "a grouped store again")
    finally:
        c.close()
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.MhError, match="no model database"):
            fresh.object_hulls([0], [pose], K, CAM, 32)
    finally:
        fresh.close()
