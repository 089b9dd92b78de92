"""tests/hull_ref.py against recorded outputs of the reference's own getConvexHull (tests/golden/hull_ref.npz, made by
tests/tools/make_hull_golden.py): the float32 restatement of the chain, and the chain behind the eight-direction
prefilter of csrc/hull.hip, both with 0 differences -- vertex values and vertex order.  That the prefiltered chain
equals the plain one is exact in exact arithmetic and a CONDITION in float: these inputs were seen to meet it."""
import os

import numpy as np
import pytest

import hull_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hull_ref.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    fam = [str(s) for s in z["families"]]
    cases = []
    for c in range(len(z["family"])):
        cases.append((fam[z["family"][c]], z["pts"][z["off"][c]:z["off"][c + 1]], z["hull"][z["hoff"][c]:z["hoff"][c + 1]]))
    return cases


def test_golden_holds_every_family(golden):
    count = {}
    for fam, pts, hull in golden:
        count[fam] = count.get(fam, 0) + 1
    assert set(count) == {"small", "empty", "equal", "collinear", "lattice", "uniform", "projected", "circle"}
    assert count["lattice"] == 300 and count["uniform"] == 300 and count["projected"] >= 20
    assert max(len(p) for f, p, h in golden if f == "projected") == 5000


def test_quirks_of_the_reference_are_in_the_golden(golden):
    for fam, pts, hull in golden:
        if len(pts) == 1:
            assert len(hull) == 0                      # one point: the empty hull
        if fam == "equal":
            assert len(hull) == 2 and np.all(hull == pts[0])   # the first and the last point of the sorted list
        if fam == "collinear":
            assert len(hull) == 2                      # the two ends (collinear and duplicate points are dropped)
            assert tuple(hull[0]) == tuple(hull_ref.sort_points(pts)[-1]) and tuple(hull[1]) == tuple(hull_ref.sort_points(pts)[0])
        if fam == "small" and len(pts) == 2 and not np.all(pts[0] == pts[1]):
            s = hull_ref.sort_points(pts)
            assert np.all(hull == s[::-1])             # two points: both, the larger first


@pytest.mark.parametrize("variant", ["chain", "chain_prefiltered"])
def test_restatement_equals_the_reference(golden, variant):
    fn = getattr(hull_ref, variant)
    differences = []
    for c, (fam, pts, hull) in enumerate(golden):
        if not hull_ref.same_vertices(fn(pts), hull):
            differences.append((c, fam, len(pts)))
    assert not differences, differences


def test_prefilter_discards_most_of_a_projected_cloud(golden):
    share = [len(hull_ref.prefilter(p)) / len(p) for f, p, h in golden if f == "projected"]
    assert np.mean(share) < 0.25, share   # (else the device's prefilter form would be tested on next to nothing)
