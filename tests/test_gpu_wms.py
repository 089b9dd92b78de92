"""moped3d's CLUSTER_WEIGHTED_MEAN_SHIFT_CPU on the GPU (moped_amd/csrc/wms.hip) through mh_cluster_wms and
mh_wms_debug_state, against what the reference's own class recorded (tests/golden/wms_ref.npz) and against the float32
restatement (tests/wms_ref.py, itself pinned to that golden by tests/test_wms_ref_cpu.py).  The kernel keeps the
reference's fp32 operation order, so everything is exact: clusters, member order, iteration counts and active flags equal,
weights and centres bit for bit (a NaN equals a NaN: wms_ref.same_floats says why)."""
import ctypes as C

import numpy as np
import pytest

import wms_ref
from moped_amd import capi
from test_wms_ref_cpu import Golden

pytestmark = pytest.mark.gpu
FAMILIES = ["sizes", "blobs", "dup", "lattice", "radius0", "iter", "fill", "nan", "images", "overlap"]


@pytest.fixture(scope="module")
def golden():
    return Golden()


def _params(c):
    return capi.mh_wms_params(c["radius"], c["merge"], c["min_pts"], c["max_iter"], c["hwd"])


def _problems(c):
    """process()'s per-image lists (:195-201): the model's matches of image i, in match order"""
    return [(c["xyz"][c["image"] == i], c["fill"][c["image"] == i]) for i in range(c["images"])]


def _same_clusters(got, want, what=""):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert np.array_equal(g, w), what   # the same members in the same (descending) order


@pytest.mark.parametrize("family", FAMILIES)
def test_clusters_and_state_equal_the_reference(ctx, golden, family):
    assert golden.families == FAMILIES
    ids = [i for i in range(golden.n) if golden.families[golden.g["family"][i]] == family]
    assert ids
    for i in ids:
        c = golden.case(i)
        what = f"case {i} ({family}, n = {len(c['xyz'])})"
        per_image = ctx.cluster_wms(_problems(c), _params(c))
        _same_clusters([cl for im in per_image for cl in im], c["clusters"], what)   # appended in image order (:202-204)
        state = ctx.wms_debug_state(_problems(c), _params(c))
        assert len(state) == len(c["state"])
        for (wt, centre, active, it), ref in zip(state, c["state"]):
            assert wms_ref.same_floats(wt, ref["weight"]), what
            assert it == ref["iterations"], what
            assert np.array_equal(active, ref["active"]), what
            assert wms_ref.same_floats(centre, ref["centre"]), what


def test_fresh_input_equals_the_restatement(ctx):
    """A scene the golden does not hold, with overlap: three blobs a little more than Radius apart."""
    rng = np.random.default_rng(77)
    ctr = np.array([[0.0, 0.0, 1.0], [0.25, 0.0, 1.0], [0.0, 0.25, 1.05]])
    xyz = (ctr[rng.integers(0, 3, 333)] + rng.normal(0, 0.03, (333, 3))).astype(np.float32)
    fill = np.where(rng.random(333) < 0.5, 0, rng.uniform(0, 40, 333)).astype(np.float32)
    R, M, min_pts, max_iter, hwd = 0.2, 0.01, 5, 37, 7.5
    prm = capi.mh_wms_params(R, M, min_pts, max_iter, hwd)
    want, C0, act0, it0 = wms_ref.weighted_mean_shift(xyz, wms_ref.cauchy_weight(fill, hwd), R, M, min_pts, max_iter)
    assert sum(len(m) for m in want) > len(xyz)   # points in several clusters
    _same_clusters(ctx.cluster_wms([(xyz, fill)], prm)[0], want)
    wt, centre, active, it = ctx.wms_debug_state([(xyz, fill)], prm)[0]
    assert it == it0 and np.array_equal(active, act0)
    assert wms_ref.same_floats(centre, C0) and wms_ref.same_floats(wt, wms_ref.cauchy_weight(fill, hwd))


def test_batch_of_mixed_sizes_equals_the_problems_alone(ctx, golden):
    """One launch, one workgroup per problem, the last one lays the CSR out: sizes 0 .. 2048 in one call."""
    cases = [golden.case(i) for i in range(golden.n)]
    same = [c for c in cases if (c["radius"], c["merge"], c["min_pts"], c["max_iter"], c["hwd"], c["images"]) ==
            (cases[0]["radius"], cases[0]["merge"], cases[0]["min_pts"], cases[0]["max_iter"], cases[0]["hwd"], 1)]
    sizes = sorted(len(c["xyz"]) for c in same)
    assert sizes[0] == 0 and sizes[-1] == 2048 and len(same) >= 12
    prm = _params(same[0])
    together = ctx.cluster_wms([(c["xyz"], c["fill"]) for c in same], prm)
    states = ctx.wms_debug_state([(c["xyz"], c["fill"]) for c in same], prm)
    for c, got, (wt, centre, active, it) in zip(same, together, states):
        _same_clusters(got, c["clusters"], f"n = {len(c['xyz'])}")
        assert it == c["state"][0]["iterations"] and np.array_equal(active, c["state"][0]["active"])
        assert wms_ref.same_floats(centre, c["state"][0]["centre"])


def test_caps_whole_clusters_only(ctx, golden):
    c = max((golden.case(i) for i in range(golden.n) if golden.families[golden.g["family"][i]] == "overlap"),
            key=lambda k: sum(len(m) for m in k["clusters"]) / len(k["xyz"]))   # the one with the most memberships per point
    prm, problems = _params(c), [(c["xyz"], c["fill"])] * 2   # two problems: the cut falls inside the second
    want = c["clusters"] + c["clusters"]
    n_k, n_m = len(want), sum(len(m) for m in want)
    assert n_m > 2 * len(c["xyz"]) and len(c["clusters"]) >= 2

    def written(cl_off, members, k):
        return [members[cl_off[j]:cl_off[j + 1]] for j in range(k)]

    # exactly fitting
    rc, ncl, cl_off, members, needed = ctx.cluster_wms_raw(problems, prm, n_k, n_m)
    assert rc == capi.MH_OK and needed == (n_k, n_m) and list(ncl) == [n_k // 2, n_k // 2]
    assert cl_off[n_k] == n_m
    _same_clusters(written(cl_off, members, n_k), want)
    # one member short: the last cluster is left out whole
    rc, ncl, cl_off, members, needed = ctx.cluster_wms_raw(problems, prm, n_k, n_m - 1)
    assert rc == capi.MH_ERR_CAPACITY and needed == (n_k, n_m)
    assert b"clusters" in ctx.L.mh_last_error(ctx.h)
    assert list(ncl) == [n_k // 2, n_k // 2 - 1]
    _same_clusters(written(cl_off, members, n_k - 1), want[:-1])
    assert (members[cl_off[n_k - 1]:] == -1).all() and (cl_off[n_k:] == -1).all()   # nothing of the cluster that did not fit
    # one cluster short
    rc, ncl, cl_off, members, needed = ctx.cluster_wms_raw(problems, prm, n_k - 1, n_m)
    assert rc == capi.MH_ERR_CAPACITY and needed == (n_k, n_m) and list(ncl) == [n_k // 2, n_k // 2 - 1]
    _same_clusters(written(cl_off, members, n_k - 1), want[:-1])
    assert (members[cl_off[n_k - 1]:] == -1).all()
    # the cut inside the first problem; no room at all
    first = len(want[0])
    rc, ncl, cl_off, members, needed = ctx.cluster_wms_raw(problems, prm, n_k, first + 1)
    assert rc == capi.MH_ERR_CAPACITY and list(ncl) == [1, 0] and cl_off[1] == first and (members[first:] == -1).all()
    rc, ncl, cl_off, members, needed = ctx.cluster_wms_raw(problems, prm, 0, 0)
    assert rc == capi.MH_ERR_CAPACITY and needed == (n_k, n_m) and list(ncl) == [0, 0] and cl_off[0] == 0
    # the context goes on: the wrapper asks again with what is needed
    _same_clusters([cl for p in ctx.cluster_wms(problems, prm) for cl in p], want)


def test_bad_arguments_are_refused(ctx):
    L, h = ctx.L, ctx.h
    rng = np.random.default_rng(3)
    n = 2049
    xyz, fill = rng.normal(0, 0.1, (n, 3)).astype(np.float32), np.zeros(n, np.float32)
    ncl, cl_off, members = np.full(4, -7, np.int32), np.full(n + 1, -7, np.int32), np.full(4 * n, -7, np.int32)
    needed = np.full(2, -7, np.int64)
    P = capi._ptr

    def call(xyz_=xyz, fill_=fill, off=(0, 100), prm=None, ncl_=ncl, cl_off_=cl_off, members_=members, caps=(n, 4 * n),
             null_prm=False):
        off = np.asarray(off, np.int32)
        prm = prm or capi.mh_wms_params()
        return L.mh_cluster_wms(h, P(xyz_), P(fill_), P(off), len(off) - 1, None if null_prm else C.byref(prm), P(ncl_),
                                P(cl_off_), caps[0], P(members_), caps[1], P(needed))

    def refused(rc, word):
        assert rc == capi.MH_ERR_ARG
        msg = L.mh_last_error(h).decode()
        assert msg.startswith("mh_cluster_wms: ") and word in msg, msg
        assert (members == -7).all() and (cl_off == -7).all() and (ncl == -7).all() and (needed == -7).all()   # nothing came back

    refused(call(off=(0, 2049)), "2048")
    refused(call(off=(0, 10, 2059)), "2048")
    refused(call(off=(0, 50, 40)), "off")
    refused(call(off=(1, 50)), "off")
    prm0 = capi.mh_wms_params()
    refused(L.mh_cluster_wms(h, P(xyz), P(fill), None, 1, C.byref(prm0), P(ncl), P(cl_off), n, P(members), 4 * n, P(needed)), "off")
    refused(call(xyz_=None), "xyz_host")
    refused(call(fill_=None), "fill_host")
    refused(call(null_prm=True), "prm")
    refused(call(ncl_=None), "n_clusters")
    refused(call(cl_off_=None), "cl_off")
    refused(call(members_=None), "members")
    refused(call(caps=(-1, 10)), "cap_")
    for field, word in (("radius", "radius"), ("merge", "merge"), ("half_weight_distance", "half_weight_distance")):
        for bad in (float("nan"), -0.5):
            prm = capi.mh_wms_params()
            setattr(prm, field, bad)
            refused(call(prm=prm), word)
    refused(call(prm=capi.mh_wms_params(max_iter=-1)), "max_iter")
    # the debug entry checks the same way
    off = np.array([0, 2049], np.int32)
    prm = capi.mh_wms_params()
    w, ctr, act, it = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros(1, np.int32)
    assert L.mh_wms_debug_state(h, P(xyz), P(fill), P(off), 1, C.byref(prm), P(w), P(ctr), P(act), P(it)) == capi.MH_ERR_ARG
    assert L.mh_last_error(h).decode().startswith("mh_wms_debug_state: ")
    # ... and 2048 points are taken
    assert call(off=(0, 2048)) == capi.MH_OK and needed[0] >= 0 and ncl[0] >= 0
