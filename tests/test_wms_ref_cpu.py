"""The float32 restatement of moped3d's weighted mean shift (tests/wms_ref.py) against what the reference's own class
recorded (tests/golden/wms_ref.npz, made by tests/tools/make_wms_golden.py): clusters, member order, weights and final
centres bit for bit (NaN = NaN, see wms_ref.same_floats), active flags and iteration counts, on every family."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wms_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wms_ref.npz")


class Golden:
    """The recorded cases.  case(i) -> dict with the inputs, `clusters` (process()'s list for the model) and `state`
    (per image: weight, centre, active, iterations)."""

    def __init__(self):
        g = np.load(GOLDEN)
        self.g = {k: g[k] for k in g.files}
        self.families = [str(f) for f in self.g["families"]]
        self.n = len(self.g["family"])
        self.k0 = np.concatenate([[0], np.cumsum(self.g["ncl"])])
        self.p0 = np.concatenate([[0], np.cumsum(self.g["iprm"][:, 2])])

    def case(self, i):
        g = self.g
        b, e = int(g["off"][i]), int(g["off"][i + 1])
        R, M, hwd = (float(v) for v in g["prm"][i])
        min_pts, max_iter, images = (int(v) for v in g["iprm"][i])
        clusters = [g["members"][g["cl_off"][k]:g["cl_off"][k + 1]] for k in range(self.k0[i], self.k0[i + 1])]
        state = []
        for p in range(self.p0[i], self.p0[i + 1]):
            pb, pe = int(g["poff"][p]), int(g["poff"][p + 1])
            state.append(dict(weight=g["weight"][pb:pe], centre=g["centre"][pb:pe], active=g["active"][pb:pe].astype(bool),
                              iterations=int(g["iterations"][p])))
        return dict(family=self.families[g["family"][i]], xyz=g["xyz"][b:e], fill=g["fill"][b:e],
                    image=g["image"][b:e].astype(np.int32), images=images, radius=R, merge=M, hwd=hwd, min_pts=min_pts,
                    max_iter=max_iter, clusters=clusters, state=state)


@pytest.fixture(scope="module")
def golden():
    return Golden()


def test_golden_covers_the_families(golden):
    g = golden.g
    assert os.path.getsize(GOLDEN) <= 300 * 1024
    assert sorted(set(golden.families[f] for f in g["family"])) == sorted(golden.families)
    sizes = set(int(n) for n in np.diff(g["off"]))
    assert {0, 1, 7, 8, 63, 64, 65, 1023, 1024, 1025, 2048} <= sizes
    assert np.isnan(g["xyz"]).any() and (g["fill"] == -1).any() and (g["fill"] > 1000).any()
    assert (g["iprm"][:, 1] == 0).any() and (g["iprm"][:, 1] == 1).any() and (g["prm"][:, 0] == 0).any()
    assert (g["iprm"][:, 2] > 1).any()
    # overlap is real: some case has more members than points
    ratio = [(g["cl_off"][golden.k0[i + 1]] - g["cl_off"][golden.k0[i]]) / max(1, g["off"][i + 1] - g["off"][i])
             for i in range(golden.n)]
    assert max(ratio) > 2.0


def test_restatement_equals_the_reference(golden):
    for i in range(golden.n):
        c = golden.case(i)
        what = f"case {i} ({c['family']}, n = {len(c['xyz'])})"
        clusters, state = wms_ref.process(c["xyz"], c["fill"], c["image"], c["images"], c["radius"], c["merge"], c["min_pts"],
                                          c["max_iter"], c["hwd"])
        assert len(clusters) == len(c["clusters"]), what
        for mine, ref in zip(clusters, c["clusters"]):
            assert np.array_equal(mine, ref), what
        assert len(state) == len(c["state"])
        for (pos, wt, C, act, it), ref in zip(state, c["state"]):
            assert len(pos) == len(ref["weight"]), what
            assert wms_ref.same_floats(wt, ref["weight"]), what
            assert it == ref["iterations"], what
            assert np.array_equal(act, ref["active"]), what
            assert wms_ref.same_floats(C, ref["centre"]), what


def test_strict_comparisons_decide(golden):
    """The lattice cases: neighbours exactly Radius (Merge) apart are outside, one ulp more and they are inside."""
    lat = [golden.case(i) for i in range(golden.n) if golden.families[golden.g["family"][i]] == "lattice"]
    exact = next(c for c in lat if c["radius"] == 0.125 and c["merge"] == 0.125)
    assert len(exact["clusters"]) == len(exact["xyz"]) and all(len(m) == 1 for m in exact["clusters"])
    assert exact["state"][0]["iterations"] == 1 and exact["state"][0]["active"].all()
    wider = next(c for c in lat if c["radius"] > 0.125 and c["merge"] == 0.125 and c["min_pts"] == 0)
    assert max(len(m) for m in wider["clusters"]) > 1
    # MinPts is strict too: the 7-point blob is dropped, the 8-point one kept
    by_n = {len(golden.case(i)["xyz"]): golden.case(i) for i in range(golden.n) if golden.families[golden.g["family"][i]] == "sizes"}
    assert by_n[7]["clusters"] == [] and [len(m) for m in by_n[8]["clusters"]] == [8]
