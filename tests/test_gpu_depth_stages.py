"""moped3d's depth front end on the device, stage by stage against the oracle (which tests/test_ref_steps_cpu.py holds
to the reference's own classes on the same inputs, tests/depth_cases.py): the patch map of depth_patch_kernel, the keep
flags of feature_density_kernel, DEPTHFILTER2 and the depth-adaptive ratio inside group_kernel through the match lists,
DEPTHMAP_PROP's lookup and Cauchy weight per match -- fetched with mh_depth_rules_debug_fetch.  Every comparison is
exact (bit patterns for floats): the kernels restate the reference's arithmetic literally under -ffp-contract=off.

Frames: a DB of 3 models x 200 rows, queries = DB rows with noise at coordinates the case chooses; ms_min_pts above
every list, so CLUSTER .. FILTER2 have nothing to do."""
import numpy as np
import pytest

import depth_cases as dc
import orclib
from moped_amd import capi, synth

pytestmark = pytest.mark.gpu
CAM0 = synth.CAM_IDENTITY
f32 = np.float32
TABLE = np.array([[0.9, 1.4, 0.6, 0.8], [1.2, 1.45, 0.55, 0.75], [0.7, 1.3, 0.65, 0.85]], f32)   # per model: maxRatioDepth,
#                                                                                    minRatioDepth, ratioLow, ratioHigh
_ids = lambda s: "x".join(map(str, s))


def _params():
    p = capi.default_frame_params()
    p.ms_min_pts = 1 << 20
    return p


def _quantile_density(dens, q):
    """A Density that drops about the fraction q of the points: halfway between two neighbouring DISTINCT finite dilated
    densities, at the gap whose share of points below it is nearest to q.  (A 3x3 dilation over a grid of 21 patches
    leaves a handful of distinct values, shared by many points each: a quantile of the points, or of the distinct
    values, sits ON one of them, where float rounding of Density*100*100 decides which way a hundred points go.  Ties
    have a test of their own.)"""
    u = np.unique(dens[np.isfinite(dens)])
    assert len(u) >= 2, "one density everywhere: no threshold splits the points"
    below = np.array([(dens <= v).sum() for v in u[:-1]]) / len(dens)
    i = int(np.argmin(np.abs(below - q)))
    return float((np.float64(u[i]) + np.float64(u[i + 1])) / 2) / 1e4


class Case:
    """One frame: map, distance map, coordinates, descriptors, and what the oracle expects of every stage."""

    def __init__(self, db, dbn, shape, Q=600, seed=0, fill_kind="mixed", feature_q=0.5, match_q=0.3, adaptive=False,
                 outside=True, sigma=0.004, feature_tie=False):
        self.shape = self.h, self.w, self.patch = shape
        h, w, patch = shape
        self.K = dc.intrinsics(h, w)
        self.img, self.marks = dc.depth_map(h, w, patch, seed)
        self.fill = dc.fill_map(h, w, fill_kind, seed)
        self.uv = dc.coords(h, w, patch, Q, seed=seed, outside=outside, aim=self.marks.values())
        self.desc, _ = dc.queries(db, Q, seed, sigma)
        self.table = TABLE if adaptive else None
        self.Q = Q
        pm = self.pm = orclib.depth_patch_inv_size(self.img, self.K, patch)
        idx, d1, d2 = orclib.match_2nn(dbn, orclib.normalize(self.desc))
        ok = idx >= 0
        self.model_nn = model = np.where(ok, db.model_of[np.maximum(idx, 0)], -1)
        # DEPTHFILTER: Density from a quantile of the dilated densities (None: off), or an exact tie
        self.feature_density, self.keep1, self.n_tied = -1.0, None, 0
        if feature_q is not None:
            dens = orclib.depthfilter_density(self.img, self.K, patch, self.uv, None, pm)
            self.feature_density = _quantile_density(dens, feature_q)
            if feature_tie:
                ties = [(v, dc.tie_density(v)) for v in np.unique(dens[np.isfinite(dens) & (dens > 0)])]
                ties = [(v, d) for v, d in ties if d is not None]
                assert ties, "no Density reproduces one of the case's densities"
                v, self.feature_density = ties[len(ties) // 2]
                self.n_tied = int((dens == v).sum())
            self.keep1 = orclib.depthfilter_keep(self.img, self.K, patch, self.feature_density, self.uv, None, pm)
            ok &= self.keep1
        with np.errstate(all="ignore"):
            quot = (d1 / d2).astype(f32)
        if adaptive:
            self.ratio_q, reach = orclib.adaptive_ratio(self.img, self.fill, self.uv, model, TABLE, dc.MAX_DEPTH,
                                                        dc.DEFAULT_DEPTH, dc.CAUCHY_SCALE)
            ok &= reach & (quot < self.ratio_q)
        else:
            ok &= quot < f32(0.8)
        qs = np.nonzero(ok)[0]
        qs = qs[np.lexsort((qs, model[qs]))]                       # matches[model] lists, ascending query
        self.match_density, self.n_dropped2 = -1.0, 0
        if match_q is not None:
            off = np.searchsorted(model[qs], np.arange(dc.N_MODELS + 1))
            dens = orclib.depthfilter_density(self.img, self.K, patch, self.uv[qs], off, pm)
            self.match_density = _quantile_density(dens, match_q)
            keep2 = orclib.depthfilter_keep(self.img, self.K, patch, self.match_density, self.uv[qs], off, pm)
            self.n_dropped2 = int((~keep2).sum())
            qs = qs[keep2]
        self.q, self.model = qs.astype(np.int32), model[qs].astype(np.int32)
        self.world, self.weight = orclib.depthmap_prop(self.img, self.fill, self.uv[qs], dc.CAUCHY_SCALE)

    def decisions(self):
        return dict(inv_size=len(self.pm[0]), keep1=0 if self.keep1 is None else self.Q, lists=self.Q, m_depth=len(self.q))


class Device:
    def __init__(self, db, reserve):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.c = capi.Context(0)
        self.c.db_upload(self.c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        self.c.reserve(reserve)
        self.keepalive = []

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keepalive.append(t)
        return t

    def set_case(self, case):
        c = self.c
        self.keepalive = []
        img, fill = self.up(case.img), (self.up(case.fill) if case.fill is not None else None)
        c.frame_set_depth_image(img.data_ptr(), fill.data_ptr() if fill is not None else 0, case.w, case.h,
                                capi.DEPTH_BACKPROJECTION, 0.5, dc.CAUCHY_SCALE)
        c.frame_set_depth_rules(case.K, case.patch, case.feature_density, case.match_density, case.table, dc.MAX_DEPTH,
                                dc.DEFAULT_DEPTH, dc.CAUCHY_SCALE)

    def run(self, case, seed=3):
        qd, uv = self.up(case.desc), self.up(case.uv)      # (the frame normalises the descriptors in place: a fresh copy)
        self.c.frame_enqueue(qd.data_ptr(), uv.data_ptr(), case.Q, case.K, CAM0, _params(), seed)
        return self.c.frame_fetch()[1]

    def close(self):
        self.c.frame_set_depth_rules(off=True)
        self.c.frame_set_depth_image(0, 0, 0, 0, 0)
        self.c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _check_stages(c, case, slot=0, what=None):
    """Frame `slot`'s three stage outputs and its match lists against the case's oracle."""
    what = what or (case.shape, slot)
    if case.feature_density >= 0 or case.match_density >= 0:
        inv = c.depth_rules_debug_fetch("inv_size", slot, len(case.pm[0]))
        assert np.array_equal(_bits(inv), _bits(case.pm[0])), (what, "inv_size", np.nonzero(_bits(inv) != _bits(case.pm[0]))[0][:8])
    if case.keep1 is not None:
        keep1 = c.depth_rules_debug_fetch("keep1", slot, case.Q)
        assert np.array_equal(keep1.astype(bool), case.keep1), (what, "keep1", np.nonzero(keep1.astype(bool) != case.keep1)[0][:8])
    q, m = c.frame_fetch_matches_slot(slot)
    assert np.array_equal(q, case.q) and np.array_equal(m, case.model), (what, "lists", len(q), len(case.q))
    md = c.depth_rules_debug_fetch("m_depth", slot, len(q))
    got_world = np.stack([md["wx"], md["wy"], md["wz"]], 1)
    assert np.array_equal(_bits(got_world), _bits(case.world)), (what, "m_depth xyz")
    assert np.array_equal(_bits(md["w"]), _bits(case.weight)), (what, "m_depth weight")


@pytest.fixture(scope="module")
def scene():
    db = dc.make_db()
    dev = Device(db, 2200)
    yield dict(db=db, dbn=orclib.normalize(db.desc), dev=dev)
    dev.close()


# ------------------------------------------------------------------------------------------------ the shapes, all stages
@pytest.mark.parametrize("fill_kind", dc.FILL_KINDS)
@pytest.mark.parametrize("shape", dc.SHAPES, ids=_ids)
def test_every_stage_equals_the_oracle(scene, shape, fill_kind):
    """Patch map, keep flags, match lists (DEPTHFILTER, the fixed ratio, DEPTHFILTER2) and per-match depth at every
    shape, with coordinates on patch boundaries, off the map (both sides clamp) and on the planted regions, without a
    distance map, with zeros and with the mixed one; a second frame gives the same (the per-(model, patch) counts are
    back to zero)."""
    dev = scene["dev"]
    case = Case(scene["db"], scene["dbn"], shape, seed=dc.FILL_KINDS.index(fill_kind), fill_kind=fill_kind)
    # the case bites: both filters keep and drop, the planted regions are hit, coordinates lie off the map
    assert 40 <= case.keep1.sum() <= case.Q - 40 and case.n_dropped2 >= 10 and len(case.q) >= 30
    assert np.isinf(case.pm[0][case.marks["zero"]]) and case.pm[0][case.marks["all_nan"]] < 1e-12 and (case.uv < 0).any()
    if fill_kind == "none":        # fillDistance -1: factor -10, weight 1 / 101
        assert (case.weight == orclib.cauchy_weight(np.array([-1], f32), dc.CAUCHY_SCALE)[0]).all()
    elif fill_kind == "zeros":
        assert (case.weight == 1).all()
    else:                          # 0, exactly CauchyScale, and values whose square overflows
        assert (case.weight == 1).any() and (case.weight == f32(0.5)).any() and (case.weight == 0).any()
    dev.set_case(case)
    for rep in range(2):
        counts = dev.run(case)
        assert counts[0] == len(case.q)
        _check_stages(dev.c, case, what=(shape, fill_kind, rep))


@pytest.mark.parametrize("shape", dc.SHAPES[:4], ids=_ids)
def test_feature_filter_at_an_exact_tie(scene, shape):
    """Density*100*100 equal to the dilated density of some features bit for bit: `>` is strict, they go -- on the
    device as in the oracle (and in the class: test_ref_steps_cpu)."""
    dev = scene["dev"]
    case = Case(scene["db"], scene["dbn"], shape, seed=0, outside=False, match_q=None, feature_tie=True)
    assert case.n_tied >= 1
    dev.set_case(case)
    dev.run(case)
    _check_stages(dev.c, case)


def test_portrait_map_takes_the_reference_y1_as_written(scene):
    """w < h: `y1 = min((py+1)*PatchSize, width)` (DEPTHFILTER_CPU.hpp:171) falls below y0 from the fourth patch row on
    and clamps in the third; the areas from there on are not what an unclamped y1 gives, and the device has the
    reference's."""
    h, w, patch = dc.SHAPES[1]
    case = Case(scene["db"], scene["dbn"], dc.SHAPES[1], seed=5, match_q=None)
    assert h > w and dc.grid(h, w, patch) == (3, 7)
    # the same depths in a map padded (with NaN, which never lowers a minimum) to 7 patches across: no y1 clamps there
    padded = np.pad(case.img, ((0, 0), (0, 7 * patch - w), (0, 0)), constant_values=np.nan)
    unclamped = orclib.depth_patch_inv_size(padded, case.K, patch)[0].reshape(7, 7)[:, :2]
    ours = case.pm[0].reshape(7, 3)[:, :2]
    assert np.array_equal(unclamped[:2], ours[:2]) and (unclamped[2:] != ours[2:]).any(axis=1).all()
    scene["dev"].set_case(case)
    scene["dev"].run(case)
    _check_stages(scene["dev"].c, case)


def test_depthmap_prop_alone_reads_every_kind_of_pixel(scene):
    """No filter, the fixed ratio: every query with a neighbour is a match, so DEPTHMAP_PROP's lookup meets the NaN
    patch and band, the zero patch, the patch beyond MaximumDepth and the negative pixel."""
    case = Case(scene["db"], scene["dbn"], dc.SHAPES[2], seed=4, feature_q=None, match_q=None)
    z = case.world[:, 2]
    assert len(case.q) > 550 and np.isnan(z).any() and (z == 0).any() and (z == 5).any() and (z < 0).any()
    scene["dev"].set_case(case)
    scene["dev"].run(case)
    _check_stages(scene["dev"].c, case)


# ------------------------------------------------------------------------------------------------------ the adaptive ratio
def test_adaptive_ratio_lists_reach_every_branch(scene):
    """MATCH_ADAPTIVE_FLANN's ratio per query inside group_kernel: the accepted lists equal orclib.adaptive_ratio's.  The
    census is taken on the oracle's side: all four branches of getRatio, a depth beyond MaximumDepth and a NaN depth
    must occur among the queries with a neighbour, and the test must accept and refuse a good many of them."""
    dev = scene["dev"]
    case = Case(scene["db"], scene["dbn"], dc.SHAPES[0], seed=7, feature_q=None, match_q=None, adaptive=True,
                sigma=(0.002, 0.06))
    ix = np.clip(case.uv[:, 0].astype(np.int32), 0, case.w - 1)
    iy = np.clip(case.uv[:, 1].astype(np.int32), 0, case.h - 1)
    depth = case.img[iy, ix, 2]
    cp = TABLE[np.maximum(case.model_nn, 0)]
    with np.errstate(invalid="ignore"):
        far = depth > dc.MAX_DEPTH
        rising = ~far & (depth < cp[:, 0])
        flat = ~far & ~rising & (depth < cp[:, 1])
        fading = ~far & ~rising & ~flat & (depth < cp[:, 1] * f32(2))
        zero = ~far & ~rising & ~flat & ~fading & ~np.isnan(depth)
    census = dict(far=int(far.sum()), rising=int(rising.sum()), flat=int(flat.sum()), fading=int(fading.sum()),
                  zero=int(zero.sum()), nan=int(np.isnan(depth).sum()))
    assert min(census.values()) >= 3, census
    acc = np.isin(np.arange(case.Q), case.q)
    assert acc[rising].any() and acc[flat].any() and acc[fading].any() and not acc[far].any()
    assert 100 < len(case.q) < case.Q - 100
    plain = Case(scene["db"], scene["dbn"], dc.SHAPES[0], seed=7, feature_q=None, match_q=None, sigma=(0.002, 0.06))
    assert not np.array_equal(plain.q, case.q)                         # (the table decides, not the fixed 0.8)
    dev.set_case(case)
    for rep in range(2):
        dev.run(case)
        _check_stages(dev.c, case, what=("adaptive", rep))


def test_all_rules_together(scene):
    dev = scene["dev"]
    case = Case(scene["db"], scene["dbn"], dc.SHAPES[2], seed=9, adaptive=True, sigma=(0.002, 0.05), match_q=0.4)
    assert case.n_dropped2 > 5 and len(case.q) > 30
    dev.set_case(case)
    dev.run(case)
    _check_stages(dev.c, case)


# ------------------------------------------------------------------------------- more matches than group_kernel keeps in LDS
def test_depth_map_and_match_filter_past_the_lds_lists(scene):
    """More than GROUP_LDS_M = 2 048 accepted matches AFTER DEPTHFILTER2, with a depth map set: group_kernel's placement
    and DEPTHMAP_PROP on the global-memory scans."""
    dev = scene["dev"]
    case = Case(scene["db"], scene["dbn"], dc.SHAPES[0], Q=2200, seed=11, feature_q=None, match_q=0.03)
    assert 2048 < len(case.q) < 2200 and case.n_dropped2 >= 10, (len(case.q), case.n_dropped2)
    dev.set_case(case)
    counts = dev.run(case)
    assert counts[0] == len(case.q)
    _check_stages(dev.c, case)


# ----------------------------------------------------------------------------------------------------------------- a batch
def test_batch_of_three_portrait_frames_with_their_own_maps():
    """mh_frame_enqueue_batch with a depth map and a distance map per frame (blockIdx.y in all three kernels) at the
    portrait shape: every slot's patch map, keep flags, lists and per-match depth equal the oracle's for THAT frame."""
    import torch
    dev = torch.device("cuda:0")
    db = dc.make_db()
    dbn = orclib.normalize(db.desc)
    shape, B, Q = dc.SHAPES[1], 3, 600
    h, w, patch = shape
    cases = [Case(db, dbn, shape, Q=Q, seed=20 + f) for f in range(B)]
    # one Density for the batch (the rules are the context's): frame 0's; the other frames' oracles follow it
    for cs in cases[1:]:
        cs.__dict__.update(_with_densities(db, dbn, cs, cases[0].feature_density, cases[0].match_density).__dict__)
    assert not np.array_equal(cases[0].pm[0], cases[1].pm[0]) and not np.array_equal(cases[1].q, cases[2].q)
    c = capi.Context(0)
    try:
        c.db_upload(c.normalize(db.desc), db.model_of, db.xyz, db.n_models)
        c.reserve_batch(Q, B)
        imgs = [torch.from_numpy(cs.img).to(dev) for cs in cases]
        fills = [torch.from_numpy(cs.fill).to(dev) for cs in cases]
        c.frame_set_depth_image_batch([t.data_ptr() for t in imgs], [t.data_ptr() for t in fills], w, h,
                                      capi.DEPTH_BACKPROJECTION, 0.5, dc.CAUCHY_SCALE)
        c.frame_set_depth_rules(cases[0].K, patch, cases[0].feature_density, cases[0].match_density, None, dc.MAX_DEPTH,
                                dc.DEFAULT_DEPTH, dc.CAUCHY_SCALE)
        qd = torch.from_numpy(np.concatenate([cs.desc for cs in cases])).to(dev)
        uv = torch.from_numpy(np.concatenate([cs.uv for cs in cases])).to(dev)
        c.frame_enqueue_batch(qd.data_ptr(), uv.data_ptr(), Q, B, cases[0].K, CAM0, _params(), [5, 6, 7])
        for f in range(B):
            _, counts = c.frame_fetch_slot(f)
            assert counts[0] == len(cases[f].q)
        for f in range(B):
            _check_stages(c, cases[f], slot=f)
    finally:
        c.close()


def _with_densities(db, dbn, case, feature_density, match_density):
    """The case's oracle again with given Densities instead of its own quantiles."""
    o = object.__new__(Case)
    o.__dict__.update(case.__dict__)
    img, K, patch, uv, pm = case.img, case.K, case.patch, case.uv, case.pm
    idx, d1, d2 = orclib.match_2nn(dbn, orclib.normalize(case.desc))
    o.feature_density, o.match_density = feature_density, match_density
    o.keep1 = orclib.depthfilter_keep(img, K, patch, feature_density, uv, None, pm)
    with np.errstate(all="ignore"):
        ok = (idx >= 0) & o.keep1 & ((d1 / d2).astype(f32) < f32(0.8))
    qs = np.nonzero(ok)[0]
    qs = qs[np.lexsort((qs, case.model_nn[qs]))]
    off = np.searchsorted(case.model_nn[qs], np.arange(dc.N_MODELS + 1))
    qs = qs[orclib.depthfilter_keep(img, K, patch, match_density, uv[qs], off, pm)]
    o.q, o.model = qs.astype(np.int32), case.model_nn[qs].astype(np.int32)
    o.world, o.weight = orclib.depthmap_prop(img, case.fill, uv[qs], dc.CAUCHY_SCALE)
    return o


# ------------------------------------------------------------------------------------------------- refusals and the fetch
def test_too_many_patches_are_refused_and_the_context_goes_on(scene):
    """(480, 640, 8): 4 800 patches do not fit feature_density_kernel's LDS arrays -- an error, nothing launched on
    them, nothing for the debug fetch to read; the next frame at a shape that fits is served as usual."""
    dev = scene["dev"]
    h, w, patch = dc.REFUSED_SHAPE
    good = Case(scene["db"], scene["dbn"], dc.SHAPES[4], seed=13)
    big = Case.__new__(Case)
    big.__dict__.update(good.__dict__)
    big.patch, big.shape = patch, dc.REFUSED_SHAPE
    assert (h, w) == (good.h, good.w) and dc.grid(h, w, patch)[0] * dc.grid(h, w, patch)[1] == 4800
    dev.set_case(big)
    with pytest.raises(capi.MhError, match="4096 patches"):
        dev.run(big)
    for which, n in (("inv_size", 4800), ("keep1", big.Q)):
        with pytest.raises(capi.MhError):
            dev.c.depth_rules_debug_fetch(which, 0, n)
    dev.set_case(good)
    dev.run(good)
    _check_stages(dev.c, good)


def test_debug_fetch_refuses_wrong_sizes_and_unset_state(scene):
    dev = scene["dev"]
    case = Case(scene["db"], scene["dbn"], dc.SHAPES[0], seed=1, feature_q=None, match_q=0.3)
    dev.set_case(case)
    dev.run(case)
    c, P = dev.c, len(case.pm[0])
    assert len(c.depth_rules_debug_fetch("inv_size", 0, P)) == P
    for which, n, slot in (("inv_size", P - 1, 0), ("inv_size", P + 1, 0), ("inv_size", P, 1), ("m_depth", len(case.q) + 1, 0),
                           ("m_depth", max(len(case.q) - 1, 0), 0), ("keep1", case.Q, 0)):     # keep1: the feature filter is off
        with pytest.raises(capi.MhError):
            c.depth_rules_debug_fetch(which, slot, n)
    c.frame_set_depth_rules(off=True)                                 # a frame without rules: no patch map to read
    dev.run(case)
    with pytest.raises(capi.MhError):
        c.depth_rules_debug_fetch("inv_size", 0, P)
    md = c.depth_rules_debug_fetch("m_depth", 0)                      # the depth map is still set: DEPTHMAP_PROP ran
    assert len(md) == len(c.frame_fetch_matches()[0]) > 0
    c.frame_set_depth_image(0, 0, 0, 0, 0)
    dev.run(case)
    with pytest.raises(capi.MhError):
        c.depth_rules_debug_fetch("m_depth", 0, len(c.frame_fetch_matches()[0]))
