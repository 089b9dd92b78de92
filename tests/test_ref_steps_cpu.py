"""The oracle against the reference's OWN step classes, each driven through its process() (oracle/ref_steps_harness.cpp
stands in for src/util.hpp and includes the headers where they lie): moped3d's DEPTHFILTER_CPU and DEPTHMAP_PROP_CPU,
CLUSTER_MEAN_SHIFT_CPU of both trees, moped2's FILTER_PROJECTION_CPU.  With these the rows "mean shift", "FILTER" and
"depth rules" of the parity table read device == oracle == the reference's code, on the inputs the device is tested
with (tests/depth_cases.py, tests/filter_cases.py) and on the witness's differential generators.  Whoever disagrees with
the class is wrong.

Skips only where oracle/_ref holds no step libraries (they are built where the reference is present and travel with
the tree)."""
import numpy as np
import pytest

import depth_cases as dc
import filter_cases
import orclib
from moped_amd import synth
from test_witness_cpu import _filter_case, _ms_case

pytestmark = pytest.mark.skipif(not orclib.ref_steps_available(), reason="oracle/_ref holds no step libraries")

f32 = np.float32
K, CAM0 = synth.K_DEFAULT, synth.CAM_IDENTITY
N_POINTS = 600
_maps = {}


def _map(shape, seed):
    """(img, marks, patch map) of a shape's map, computed once: the Python oracle loops over the patches."""
    key = (shape, seed)
    if key not in _maps:
        h, w, patch = shape
        img, marks = dc.depth_map(h, w, patch, seed)
        _maps[key] = (img, marks, orclib.depth_patch_inv_size(img, dc.intrinsics(h, w), patch))
    return _maps[key]


# ------------------------------------------------------------------------------------------------------------ DEPTHFILTER
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthfilter_oracle_equals_the_class_in_both_modes(shape):
    """orclib.depthfilter_keep == DEPTHFILTER_CPU::process, decision for decision, ToFilter = 1 and 2.  Density comes
    from quantiles of the oracle's dilated densities, so both verdicts are well represented: in the shape's cases
    together at least 15 % kept and 15 % dropped AS THE CLASS DECIDES.  Per shape 2 maps x 2 coordinate sets x 2 modes
    x 3 quantiles = 24 cases of 600 points = 14 400 decisions; 72 000 over the five shapes."""
    h, w, patch = shape
    Kd = dc.intrinsics(h, w)
    kept = total = 0
    for mseed in range(2):
        img, marks, pm = _map(shape, mseed)
        assert np.isinf(pm[0][marks["zero"]]) and pm[0][marks["all_nan"]] < 1e-12      # area 0; the untouched 1e10
        for cseed in range(2):
            uv = dc.coords(h, w, patch, N_POINTS, seed=10 * mseed + cseed, aim=marks.values())
            for off in (None, dc.groups(N_POINTS, seed=cseed)):
                dens = orclib.depthfilter_density(img, Kd, patch, uv, off, pm)
                for qt in (0.25, 0.5, 0.75):
                    density = float(np.quantile(dens[np.isfinite(dens)], qt)) / 1e4
                    want = orclib.ref_depthfilter_keep(img, Kd, patch, density, uv, off)
                    got = orclib.depthfilter_keep(img, Kd, patch, density, uv, off, pm)
                    assert np.array_equal(got, want), (shape, mseed, cseed, off is None, qt, np.nonzero(got != want)[0][:10])
                    kept += int(want.sum())
                    total += len(want)
                assert np.isinf(dens).any()                       # features on the zero-depth patch: always kept
    assert total == 24 * N_POINTS
    assert 0.15 * total <= kept <= 0.85 * total, (shape, kept, total)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthfilter_exact_tie_is_dropped_by_the_class_and_by_the_oracle(shape):
    """A Density whose Density*100*100 equals a patch's dilated density bit for bit: the comparison is a strict `>`
    (:203, :236), the points of that density go.  Searched over the distinct densities of the case (40 ulp either side
    of density / 1e4 each); at least one tie per shape must be found."""
    h, w, patch = shape
    Kd = dc.intrinsics(h, w)
    img, marks, pm = _map(shape, 0)
    found = 0
    for off in (None, dc.groups(N_POINTS, seed=0)):
        uv = dc.coords(h, w, patch, N_POINTS, seed=0, aim=marks.values())
        dens = orclib.depthfilter_density(img, Kd, patch, uv, off, pm)
        tried = 0
        for v in np.unique(dens[np.isfinite(dens) & (dens > 0)]):
            d = dc.tie_density(v)
            if d is None:
                continue
            assert orclib.density_filter(d) == v
            want = orclib.ref_depthfilter_keep(img, Kd, patch, d, uv, off)
            got = orclib.depthfilter_keep(img, Kd, patch, d, uv, off, pm)
            assert np.array_equal(got, want), (shape, v)
            assert (dens == v).any() and not want[dens == v].any(), (shape, v)      # the class drops the tie
            assert np.array_equal(want, dens > v)
            found += 1
            tried += 1
            if tried >= 4:
                break
    assert found >= 1, shape


# ---------------------------------------------------------------------------------------------------------- DEPTHMAP_PROP
@pytest.mark.parametrize("fill_kind", dc.FILL_KINDS)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthmap_prop_lookups_equal_the_class(shape, fill_kind):
    """orclib.depthmap_lookup (what orclib.depthmap_prop reads from the maps) == DEPTHMAP_PROP_CPU::process:
    depthData.coord3D, .depth and .fillDistance as bit patterns, with a distance map and without one (-1).  The Cauchy
    weight that depthmap_prop derives from fillDistance is NOT pinned here: getCauchyWeight lives in the POSE header
    (POSE_RANSAC_LM_DIFF_BACKPROJECTION_DEPTH_CPU.hpp:194-197), which needs levmar and the RANSAC skeleton around it;
    orclib.cauchy_weight stays a restatement of that one line."""
    h, w, patch = shape
    img, marks, _ = _map(shape, 0)
    fill = dc.fill_map(h, w, fill_kind, seed=1)
    uv = dc.coords(h, w, patch, N_POINTS, seed=3, aim=marks.values())
    xyz, depth, fd, valid = orclib.ref_depthmap_prop(img, fill, uv)
    world, o_fd = orclib.depthmap_lookup(img, fill, uv)
    assert np.array_equal(world.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(world[:, 2].view(np.uint32), depth.view(np.uint32))
    assert np.array_equal(o_fd.view(np.uint32), fd.view(np.uint32))
    ix, iy = uv[:, 0].astype(int), uv[:, 1].astype(int)
    assert np.array_equal(valid, img[iy, ix, 3] >= 0)
    assert np.isnan(depth).any() and (depth == 0).any() and (depth > dc.MAX_DEPTH).any()     # the planted regions are hit
    if fill_kind == "none":
        assert (fd == -1).all()
    elif fill_kind == "mixed":
        assert (fd == f32(dc.CAUCHY_SCALE)).any() and (fd >= 1e6).any() and (fd == 0).any()
    # and depthmap_prop hands the same world points on
    assert np.array_equal(orclib.depthmap_prop(img, fill, uv, dc.CAUCHY_SCALE)[0].view(np.uint32), xyz.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- mean shift
def _as_lists(clusters):
    return [list(map(int, c)) for c in clusters]


@pytest.mark.parametrize("block", range(4))
def test_meanshift_oracle_equals_the_classes(block):
    """The witness's generator (test_witness_cpu._ms_case, same seeds: 4 x 2 600 cases, all of them): partitions,
    cluster order and the order inside every cluster exact.  2-D cases through moped2's class AND moped3d's, 3-D cases
    through moped3d's use3D branch."""
    rng = np.random.default_rng([0x3E4, block])
    n3d = multi = 0
    for case in range(2600):
        pts, radius, merge, min_pts, max_iter = _ms_case(rng)
        want = _as_lists(orclib.meanshift(pts, radius, merge, min_pts, max_iter)[0])
        trees = (2, 3) if pts.shape[1] == 2 else (3,)
        for tree in trees:
            got, models = orclib.ref_meanshift_step(pts, radius=radius, merge=merge, min_pts=min_pts, max_iter=max_iter, tree=tree)
            assert _as_lists(got) == want, (block, case, tree)
            assert not models.any()
        n3d += pts.shape[1] == 3
        multi += len(want) > 1
    assert n3d > 200 and multi > 300


def test_meanshift_process_goes_model_by_model_and_image_by_image():
    """process() (:182-199): the clusters of a model = MeanShift of its matches in image 0, then image 1, ...; member
    numbers are positions in the MODEL's match list."""
    rng = np.random.default_rng(0x3E5)
    for case in range(200):
        n_models, n_images = int(rng.integers(1, 5)), int(rng.integers(1, 4))
        off = np.concatenate([[0], np.cumsum(rng.integers(0, 40, n_models))]).astype(np.int32)
        n = int(off[-1])
        pts = (rng.uniform(0, 300, (max(1, n // 5 + 1), 2))[rng.integers(0, max(1, n // 5 + 1), n)] + rng.normal(0, 6, (n, 2))).astype(f32)
        image_of = rng.integers(0, n_images, n).astype(np.int32)
        got, models = orclib.ref_meanshift_step(pts, image_of, off, n_images, 60.0, 12.0, 3, 100, tree=2 + case % 2)
        want, want_m = [], []
        for m in range(n_models):
            for i in range(n_images):
                pos = np.nonzero(image_of[off[m]:off[m + 1]] == i)[0]
                for cl in orclib.meanshift(pts[off[m]:off[m + 1]][pos], 60.0, 12.0, 3, 100)[0]:
                    want.append([int(pos[k]) for k in cl])
                    want_m.append(m)
        assert _as_lists(got) == want and list(map(int, models)) == want_m, case


# ----------------------------------------------------------------------------------------------------------------- FILTER
def _same_filter(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what          # scores as bit patterns
    assert np.array_equal(got[1], want[1]) and list(map(int, got[2])) == list(map(int, want[2])), what
    assert _as_lists(got[3]) == _as_lists(want[3]), what


@pytest.mark.parametrize("block", range(4))
def test_filter_oracle_equals_the_class(block):
    """The witness's generator (test_witness_cpu._filter_case, same seeds: 4 x 2 600 cases, all of them; MinPoints 0..8,
    MinScore 0 / 1e-4 / 2 / 3, image coordinates shared inside and across models in 60 % of the cases): scores bitwise,
    survivors, their order and the rewritten clusters exact."""
    rng = np.random.default_rng([0xF17, block])
    kept = erased = shared = 0
    for case in range(2600):
        uv, xyz, model_off, obj_model, obj_pose, min_points, fdist, min_score = _filter_case(rng)
        want = orclib.ref_filter_step(uv, xyz, model_off, obj_model, obj_pose, K, CAM0, min_points, fdist, min_score)
        got = orclib.filter_projection(uv, xyz, model_off, obj_model, obj_pose, K, CAM0, min_points, fdist, min_score)
        _same_filter(got, want, (block, case))
        kept += int(want[1].sum())
        erased += len(want[1]) - int(want[1].sum())
        shared += len(uv) > len(np.unique(uv, axis=0))
    assert kept > 500 and erased > 500 and shared > 300


def test_filter_min_points_and_min_score_boundaries():
    """`size < MinPoints || score < MinScore` erases (:152): an object whose rewritten cluster has exactly MinPoints
    members stays and goes at MinPoints + 1; one whose score equals MinScore bit for bit stays and goes at the next
    float.  Asserted on the class's own verdicts, and the oracle must agree on all of it."""
    rng = np.random.default_rng(0xF18)
    done = 0
    for case in range(400):
        uv, xyz, model_off, obj_model, obj_pose, _, fdist, _ = _filter_case(rng)
        if not len(obj_model):
            continue
        base = orclib.ref_filter_step(uv, xyz, model_off, obj_model, obj_pose, K, CAM0, 0, fdist, 0.0)
        assert base[1].all()                                       # MinPoints 0, MinScore 0: nothing is erased
        o = int(rng.integers(0, len(obj_model)))
        size, score = len(base[3][list(base[2]).index(o)]), base[0][o]
        for min_points, min_score, stays in ((size, 0.0, True), (size + 1, 0.0, False), (0, float(score), True),
                                             (0, float(np.nextafter(score, f32(np.inf))), False)):
            want = orclib.ref_filter_step(uv, xyz, model_off, obj_model, obj_pose, K, CAM0, min_points, fdist, min_score)
            got = orclib.filter_projection(uv, xyz, model_off, obj_model, obj_pose, K, CAM0, min_points, fdist, min_score)
            _same_filter(got, want, (case, min_points, min_score))
            assert bool(want[1][o]) == stays, (case, min_points, min_score, size, score)
        done += 1
    assert done > 300


@pytest.mark.parametrize("n_images", [1, 2])
def test_filter_oracle_equals_the_class_at_the_device_sizes(n_images):
    """The cases the device's FILTER is tested with (tests/filter_cases.py: more than 256 objects, models of more than
    2 048 matches, equal scores, (0.0, y) against (-0.0, y)), single camera and two cameras: a fixed-seed subset of 40
    cases each (the class walks std::map per match and object)."""
    rng = np.random.default_rng([0xF17F, n_images])
    reached = filter_cases.Regimes()
    for case in range(40):
        c = filter_cases.make_case(rng, n_images=n_images, work=60_000)
        got = filter_cases.oracle(c)
        want = orclib.ref_filter_step(c["uv"], c["xyz"], c["model_off"], c["obj_model"], c["obj_pose"], c["Ks"], c["cams"],
                                      c["min_points"], c["fd"], c["min_score"], image_of=c["img"])
        _same_filter(got, want, (n_images, case))
        reached.add(c, got)
    assert reached.signed_zero_owned and reached.big_cluster, vars(reached)
