"""The inputs of tests/test_gpu_cluster_frame.py bite -- CPU side, before the device is trusted: every case has what it
claims (sizes, cluster counts, chunk positions), and every deliberately wrong table of tests/cluster_frame_cases.py that
applies to a case differs from the right one, so the GPU test on that case cannot pass with that defect."""
from collections import Counter

import numpy as np
import pytest

import cluster_frame_cases as cs


def _per_model(tab):
    return Counter(m for m, _, _ in tab)


def _well_formed(fr, tab, prm):
    """Rows in (model, position) order, member slots contiguous inside each unit's list, every member once."""
    us = cs.units(fr)
    assert [r[0] for r in tab] == sorted(r[0] for r in tab)
    assert [r[1] for r in tab] == sorted(r[1] for r in tab)
    for u in us:
        rows = [r for r in tab if u[3] <= r[1] < u[3] + len(u[4]) and r[0] == u[1]]
        mem = [i for r in rows for i in r[2]]
        assert len(mem) == len(set(mem)) and all(0 <= i < len(u[4]) for i in mem)
        assert all(len(r[2]) >= prm["min_pts"] for r in rows)


def test_layouts_are_the_single_problem_tests():
    import test_gpu_steps
    for kind in ("blobs", "uniform", "chain", "tight"):
        for n in (1, 7, 65):
            want = test_gpu_steps._ms_points(np.random.default_rng(n), kind, n)
            assert np.array_equal(cs.layout(np.random.default_rng(n), kind, n), want)
    p = cs.points(48, "grid90", 1)
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)) + 1e9 * np.eye(48)
    assert len(np.unique(p, axis=0)) == 48 and d.min() == 90.0      # radius 40: nobody has a neighbour


def test_frames_are_interleaved_and_in_list_order():
    fr = cs.case_a()
    e = fr.e
    # accepted queries of the models interleaved: neighbours in query order are of different models about as often as
    # two random draws are, 1 - sum (n_m / M)^2 (0.88 with four lists of a thousand or two among 11 163 matches)
    order = np.argsort(e["q"], kind="stable")
    chance = 1.0 - float(((fr.sizes() / e["n"]) ** 2).sum())
    assert chance > 0.85 and np.count_nonzero(np.diff(e["model"][order]) != 0) > 0.97 * chance * e["n"]
    # uv of a model's queries = its layout, in list order; d1 = 0.1 d2; the filler is refused
    for m, s in fr.spec.items():
        q = e["q"][e["off"][m]:e["off"][m + 1]]
        assert np.all(np.diff(q) > 0) and np.array_equal(fr.uv[q], cs.points(*s))
    assert np.array_equal(e["d1"][e["q"]], np.float32(0.1) * e["d2"][e["q"]])
    assert fr.Q - e["n"] > 500 and np.count_nonzero(e["idx"] >= 0) > e["n"] + 300


def test_case_a_mixed_sizes():
    fr, prm = cs.case_a(), cs.DEFAULT
    tab = cs.table(fr)
    _well_formed(fr, tab, prm)
    sz = fr.sizes()
    assert set(sz.tolist()) >= {0, 1, 6, 7, 8, 40, 64, 65, 150, 400, 1024, 1025, 2047, 2048}
    assert {s[1] for s in fr.spec.values()} == {"blobs", "uniform", "chain", "tight"}
    assert fr.n_models == 62 and fr.e["n"] == 11163 and len(tab) == 159
    per = _per_model(tab)
    by = {(s[0], s[1]): m for m, s in fr.spec.items()}
    assert per[by[(7, "tight")]] == 1 and per[by[(6, "tight")]] == 0            # the MinPts boundary
    assert 21 <= per[by[(400, "uniform")]] <= 24
    assert per[by[(2048, "uniform")]] >= 30 and per[by[(2048, "blobs")]] >= 2   # a full list is clustered
    assert max(len(r[2]) for r in tab) > 1000
    # more models with work than any grid has workgroups: every workgroup of every grid takes several
    b = cs.busy(fr)
    assert len(b) == cs.N_BUSY_A > 48
    for G in cs.GRIDS_A:       # leftovers in LDS: 2048 points, then 7 on the same workgroup -- and the other way round
        pairs = {(int(sz[b[r]]), int(sz[b[r + G]])) for r in range(len(b) - G)}
        assert (2048, 7) in pairs and (7, 2048) in pairs, G
    assert cs.wrong_skip(fr) != tab
    for G in range(2, 49):
        assert cs.wrong_walk_order(fr, G) != tab, G
    assert cs.other_frames_lists(fr, cs.one_busy()) != tab


def test_case_b_more_than_1024_models():
    fr = cs.case_b()
    tab = cs.table(fr)
    _well_formed(fr, tab, cs.DEFAULT)
    per = _per_model(tab)
    assert fr.n_models == 2500 and fr.Q == 12000
    assert all(per[m] >= 1 for m in cs.NAMED_B)
    assert [m // cs.CHUNK for m in cs.NAMED_B] == [0, 0, 1, 1, 1, 2, 2]
    sz = fr.sizes()
    assert len(cs.busy(fr)) == 27 and len(per) >= 15
    assert np.count_nonzero((sz > 0) & (sz < 7)) == 300 and np.count_nonzero(sz == 0) > 2000
    assert cs.wrong_first_chunk_only(fr) != tab
    assert len(cs.wrong_first_chunk_only(fr)) < len([r for r in tab if r[0] < 2048]) < len(tab)   # each chunk adds rows
    assert cs.wrong_skip(fr) != tab
    for G in (2, 4, 8, 26):       # (a grid of 27 or more gives every model with work a workgroup of its own)
        assert cs.wrong_walk_order(fr, G) != tab, G


def test_case_c_n_clusters_in_n_points():
    fr = cs.case_c()
    tab = cs.table(fr, cs.PRM_C)
    _well_formed(fr, tab, cs.PRM_C)
    assert _per_model(tab) == Counter(cs.SIZES_C) and {len(r[2]) for r in tab} == {1}
    assert set(cs.SIZES_C.values()) == {1, 2, 9, 48}
    assert all(m in cs.SIZES_C for m in (3, 4, 5)) and max(cs.SIZES_C) == fr.n_models - 1
    # every member slot of the frame's list starts a cluster: rows begin at 0, 1, 2, ...
    assert [r[1] for r in tab] == list(range(fr.e["n"]))
    assert cs.wrong_skip(fr, cs.PRM_C) != tab
    assert len(cs.busy(fr, cs.PRM_C)) == 8
    for G in (2, 4, 7):
        assert cs.wrong_walk_order(fr, G, cs.PRM_C) != tab, G
    assert cs.table(fr, cs.DEFAULT) != tab


def test_case_d_parameters_change_the_table():
    fr = cs.case_d()
    tabs = {k: cs.table(fr, p) for k, p in cs.PRMS_D.items()}
    for k, t in tabs.items():
        _well_formed(fr, t, cs.PRMS_D[k])
    of = lambda t, m: [r for r in t if r[0] == m]
    for m in (0, 2, 4):      # uniform-400, seeds 0..2: the iteration cap and the radius change each of them
        for k in ("iter1", "iter2", "r60"):
            assert of(tabs[k], m) != of(tabs["iter100"], m), (m, k)
        assert of(tabs["iter1"], m) != of(tabs["iter2"], m)
    per = _per_model(tabs["r60"])
    assert per[3] == 1 and per[6] == 1 and _per_model(tabs["iter100"])[3] == 0     # MinPts 3 reaches the kernel
    for k, p in cs.PRMS_D.items():
        assert cs.wrong_walk_order(fr, 2, p) != tabs[k]


def test_batch_e_frames_differ():
    frs = cs.batch_e()
    tabs = [cs.table(fr) for fr in frs]
    assert [fr.e["n"] for fr in frs] == [0, 11163, 158, 69] and [len(t) for t in tabs] == [0, 159, 4, 0]
    assert len({fr.Q for fr in frs}) == 1 and len({fr.n_models for fr in frs}) == 1
    assert len(cs.busy(frs[2])) == 1 and len(cs.busy(frs[3])) == 0 and frs[3].sizes().max() == 6
    for f in range(4):
        for h in range(4):
            if f != h:      # another frame's lists: other matches, and -- unless both frames have nothing to cluster --
                assert not np.array_equal(frs[f].e["q"], frs[h].e["q"])            # another table
                assert {f, h} == {0, 3} or cs.other_frames_lists(frs[f], frs[h]) != tabs[f], (f, h)


@pytest.mark.parametrize("n_images", [2, 8])
def test_case_f_several_cameras(n_images):
    fr = cs.case_f(n_images)
    tab = cs.table(fr)
    _well_formed(fr, tab, cs.DEFAULT)
    us = cs.units(fr)
    assert len(us) == fr.n_models * n_images and [u[0] for u in us] == list(range(len(us)))
    assert [u[3] for u in us] == sorted(u[3] for u in us) and us[-1][3] + len(us[-1][4]) == fr.e["n"]
    spread = [len({int(i) for i in fr.q_img[fr.e["q"][fr.e["off"][m]:fr.e["off"][m + 1]]]}) for m in range(fr.n_models)]
    assert sum(s >= 2 for s in spread) >= 10 and max(spread) == n_images
    # the shared model: fewer clusters together than per image
    per, across = _per_model(tab), _per_model(cs.wrong_across_images(fr))
    assert per[cs.SHARED_F] == 5 and across[cs.SHARED_F] == 3
    # a pair of exactly MinPts points (one cluster) and one of MinPts - 1 (none)
    ex = [len(u[4]) for u in us if u[1] == cs.EXACT_F]
    assert ex[:2] == [7, 6] and not any(ex[2:]) and per[cs.EXACT_F] == 1
    assert len(_per_model(tab)) >= 9 and max(per.values()) >= 2 * (n_images == 2) + 5
    assert cs.wrong_pair_as_model(fr) != tab and cs.wrong_across_images(fr) != tab and cs.wrong_skip(fr) != tab
    n_busy = len(cs.busy(fr))
    assert n_busy == {2: 20, 8: 53}[n_images]
    for G in (2, 4, 8, 19, 48):   # (grids below the number of pairs with work: a larger one walks them in model order)
        assert G >= n_busy or cs.wrong_walk_order(fr, G) != tab, G


def test_case_g_caps():
    for k in (3, 4):
        fr = cs.case_g(k)
        assert len(cs.table(fr)) == k and len(cs.busy(fr)) == k
    over, after = cs.case_g_over_cap(), cs.case_g_after_cap()
    assert over.sizes().max() == cs.MS_CAP + 1 and after.sizes().max() == cs.MS_CAP
    with pytest.raises(AssertionError, match="ERR_MS_CAP"):
        cs.table(over)
    assert len(cs.table(after)) == 35
