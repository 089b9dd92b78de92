"""Frames for the frame form of mean shift (meanshift_models_kernel + layout_cluster_table, the CLUSTER step of the
default frame path) and the cluster tables the oracle gives for them -- plain Python, no GPU.

A frame is built from per-model point sets: the accepted queries of all models are interleaved in random query order
(d1 = 0.1 d2), every other query is refused in the ways group_ref.make_frame knows, and the pixels of model m's queries
are the layout's points in list (ascending query) order.  `table` is the frame's cluster table as the reference's
CLUSTER_MEAN_SHIFT_CPU::process leaves it: per model -- per (model, image) pair in (model, image) order for a frame with
several cameras -- orclib.meanshift on the list's pixels, models with fewer points than MinPts skipped.

The `wrong_*` functions are deliberately wrong tables: what a kernel with one plausible defect would write.
tests/test_cluster_frame_cases_cpu.py shows, case by case, that each of them differs from the right table -- so a GPU
test that passes on a case could not pass with that defect."""
from __future__ import annotations

import functools

import numpy as np

import group_ref as g
import orclib

F32 = np.float32
MS_CAP = 2048            # points one mean-shift problem holds (meanshift.hip)
CHUNK = 1024             # models meanshift_models_kernel and layout_cluster_table take at a time (MS_THREADS)
RATIO = 0.8
DEFAULT = dict(radius=200.0, merge=20.0, min_pts=7, max_iter=100)
# what frame_rest.hip sizes the CLUSTER launch of case a's three runs to: a fresh context, after the feedback of ~50
# models with work, after a frame with one (the tests cannot see the grid; CASE a is ordered for every one of these)
GRIDS_A = (8, 48, 4)


# ---- point layouts ----------------------------------------------------------------------------------------------
def layout(rng, kind, n):
    """The layouts of tests/test_gpu_steps.py (_ms_points: blobs, uniform, chain, tight) and `grid90`: n points of a
    90-pixel grid in random order -- with radius 40 / merge 20 every point is a cluster of its own."""
    if kind == "blobs":
        c = rng.uniform([50, 50], [590, 430], size=(4, 2))
        p = c[rng.integers(0, 4, n)] + rng.normal(0, 25, size=(n, 2))
    elif kind == "uniform":
        p = rng.uniform([0, 0], [640, 480], size=(n, 2))
    elif kind == "chain":
        t = np.sort(rng.uniform(0, 1, n))
        p = np.stack([40 + 560 * t, 240 + 30 * np.sin(9 * t)], 1) + rng.normal(0, 3, (n, 2))
    elif kind == "tight":
        p = rng.normal([320, 240], 6, size=(n, 2))
    elif kind == "grid90":
        gr = np.stack(np.meshgrid(np.arange(7) * 90.0, np.arange(7) * 90.0), -1).reshape(-1, 2)
        p = gr[rng.permutation(len(gr))[:n]] + 20
    else:
        raise ValueError(kind)
    return p.astype(F32)


def points(size, kind, seed):
    return layout(np.random.default_rng([0xC5, seed]), kind, size) if size else np.zeros((0, 2), F32)


# ---- the frame builder ------------------------------------------------------------------------------------------
class Frame:
    """words [1][3][Q] / uv [Q, 2] / q_img [Q] or None to inject; e = group_ref.expected of them (the match lists)."""

    def __init__(self, db, words, uv, q_img, n_images, spec):
        self.db, self.words, self.uv, self.q_img, self.n_images, self.spec = db, words, uv, q_img, n_images, spec
        self.Q = words.shape[2]
        self.n_models = db["n_models"]
        self.e = g.expected(words, uv, db["model_of"], db["xyz"], self.n_models, RATIO, q_img=q_img)

    def sizes(self):
        return np.diff(self.e["off"])


@functools.lru_cache(maxsize=None)
def make_db(n_models):
    db = g.make_db(n_models, seed=n_models, rows_max=1)     # row r = model r
    assert np.array_equal(db["model_of"], np.arange(n_models))
    return db


def build_frame(n_models, Q, spec, seed, n_images=0):
    """spec: {model: (size, layout, seed)} or {model: (points [n, 2], images [n] or None)}; every other model gets no match.
    -> Frame."""
    db = make_db(n_models)
    rng = np.random.default_rng([0xC1, seed])
    words, uv = g.make_frame(db, Q, 0, seed=seed)           # Q refused queries (no neighbour, equal distances, the
    words = words.copy()                                    # quotient on the ratio, a row of no shard)
    idx, d1, d2 = words[0, 0], words[0, 1].view(F32), words[0, 2].view(F32)
    pts = {}
    for m, s in spec.items():
        p, im = (points(*s), None) if isinstance(s[1], str) else s
        pts[m] = (np.asarray(p, F32).reshape(-1, 2), im)
    models = np.array(sorted(pts), np.int64)
    sizes = np.array([len(pts[m][0]) for m in models], np.int64)
    M = int(sizes.sum())
    assert M <= Q and (len(models) == 0 or models.max() < n_models)
    acc = np.sort(rng.choice(Q, M, replace=False))
    owner = rng.permutation(np.repeat(models, sizes))      # accepted queries of all models interleaved
    idx[acc] = owner
    d2[acc] = rng.uniform(0.5, 2.0, M).astype(F32)
    d1[acc] = F32(0.1) * d2[acc]
    q_img = rng.integers(0, n_images, Q).astype(np.int32) if n_images else None
    for m in models:
        qs = acc[owner == m]                                # ascending: the model's list order
        uv[qs] = pts[m][0]
        if pts[m][1] is not None:
            q_img[qs] = pts[m][1]
    fr = Frame(db, words, uv, q_img, n_images, spec)
    assert fr.e["n"] == M and np.array_equal(fr.sizes()[models], sizes)
    return fr


# ---- the expected table and its wrong variants ------------------------------------------------------------------
def units(fr, per_image=True):
    """What CLUSTER clusters one after the other: (unit index, model, image, first position in the frame's list, pixels)
    per model -- per (model, image) pair in (model, image) order, the pair's matches in ascending query order (positions
    then count through the (model, image, query) copy of the lists)."""
    e, off = fr.e, fr.e["off"]
    ni = fr.n_images if (per_image and fr.n_images > 1) else 1
    out = []
    for m in range(fr.n_models):
        q = e["q"][off[m]:off[m + 1]]
        if ni == 1:
            out.append((m, m, 0, int(off[m]), fr.uv[q]))
            continue
        base = int(off[m])
        for i in range(ni):
            qi = q[fr.q_img[q] == i]
            out.append((m * ni + i, m, i, base, fr.uv[qi]))
            base += len(qi)
    return out


_ORACLE = {}


def _cluster(u, prm, skip):
    n = len(u[4])
    if n == 0 or skip(n, prm["min_pts"]):
        return []
    assert n <= MS_CAP, "the frame form truncates such a list and flags ERR_MS_CAP: no table to expect"
    key = (u[4].tobytes(), prm["radius"], prm["merge"], prm["min_pts"], prm["max_iter"])
    if key not in _ORACLE:      # (the oracle once per list and parameter set, whichever table asks)
        cl, _ = orclib.meanshift(u[4], prm["radius"], prm["merge"], prm["min_pts"], prm["max_iter"])
        _ORACLE[key] = [c.tolist() for c in cl]
    return _ORACLE[key]


def _rows(us, prm, skip=lambda n, mp: n < mp, name=lambda u: u[1]):
    rows = []
    for u in us:
        w = u[3]
        for c in _cluster(u, prm, skip):
            rows.append((name(u), w, tuple(c)))     # (cl_model, cl_begin, members inside the unit's list)
            w += len(c)
    return rows


def table(fr, prm=DEFAULT):
    """The frame's cluster table: rows (cl_model, cl_begin, members) in (model[, image], emission) order; cl_count =
    len(members), cl_begin = absolute position of the cluster's first member slot in the frame's list."""
    return _rows(units(fr), prm)


def busy(fr, prm=DEFAULT):
    """Unit indices with work, in the order the kernel's running rank counts them."""
    return [u[0] for u in units(fr) if len(u[4]) >= max(1, prm["min_pts"])]


def wrong_skip(fr, prm=DEFAULT):
    """The linkage clusterer's rule: lists of n <= MinPts points skipped."""
    return _rows(units(fr), prm, skip=lambda n, mp: n <= mp)


def wrong_pair_as_model(fr, prm=DEFAULT):
    """cl_model = the (model, image) pair's index, not divided by the images."""
    return _rows(units(fr), prm, name=lambda u: u[0])


def wrong_across_images(fr, prm=DEFAULT):
    """Clustered per model, all images together."""
    return _rows(units(fr, per_image=False), prm)


def wrong_first_chunk_only(fr, prm=DEFAULT):
    """Units from 1024 upward never looked at."""
    return _rows([u for u in units(fr) if u[0] < CHUNK], prm)


def wrong_walk_order(fr, G, prm=DEFAULT):
    """Rows in the order the workgroups come by: workgroup rank % G after workgroup, not by model."""
    us = {u[0]: u for u in units(fr)}
    order = sorted(enumerate(busy(fr, prm)), key=lambda t: (t[0] % G, t[0]))
    return _rows([us[i] for _, i in order], prm)


def other_frames_lists(fr, other, prm=DEFAULT):
    """The table of another frame's lists (a batch whose workgroup read the wrong arena)."""
    return table(other, prm)


# ---- the cases --------------------------------------------------------------------------------------------------
N_A, Q_A = 62, 12000
_BIG = {0: (2048, "uniform"), 49: (2048, "blobs")}                       # by rank among the models with work
_SEVEN = (1, 4, 8, 41, 45, 48)                                           # tight-7: one cluster of 7
_NAMED = {2: (2047, "chain"), 5: (1025, "uniform"), 11: (1024, "blobs"), 17: (400, "uniform"), 23: (400, "blobs"),
          29: (150, "blobs"), 30: (150, "uniform"), 31: (150, "chain"), 32: (150, "tight"), 50: (7, "uniform"),
          51: (7, "blobs"), 52: (65, "tight")}
_FILL = [(8, "blobs"), (40, "uniform"), (64, "chain"), (65, "tight"), (8, "uniform"), (40, "chain"), (64, "tight"),
         (65, "blobs"), (8, "chain"), (40, "tight"), (64, "blobs"), (65, "uniform"), (8, "tight"), (40, "blobs"),
         (64, "uniform"), (65, "chain")]
_IDLE_BEFORE = {0: (0, "tight"), 1: (6, "tight"), 4: (1, "uniform"), 12: (6, "uniform"), 20: (0, "blobs"),
                33: (1, "tight"), 49: (6, "blobs"), 50: (6, "chain")}   # a model without work before the rank
N_BUSY_A = 53


def spec_a():
    """~60 models of mixed sizes: more than 48 have work, so a workgroup of any grid takes several; for every grid in
    GRIDS_A a 2048-point model is directly followed by a 7-point one on the same workgroup and the other way round."""
    spec, m, fill = {}, 0, 0
    for r in range(N_BUSY_A):
        if r in _IDLE_BEFORE:
            spec[m] = _IDLE_BEFORE[r] + (100 + m,)
            m += 1
        if r in _BIG:
            s = _BIG[r]
        elif r in _SEVEN:
            s = (7, "tight")
        elif r in _NAMED:
            s = _NAMED[r]
        else:
            s = _FILL[fill % len(_FILL)]
            fill += 1
        spec[m] = s + (100 + m,)
        m += 1
    spec[m] = (0, "tight", 0)       # the DB's last model: nothing
    assert m + 1 == N_A, m + 1
    return spec


@functools.lru_cache(maxsize=None)
def case_a():
    return build_frame(N_A, Q_A, spec_a(), seed=1)


@functools.lru_cache(maxsize=None)
def one_busy(seed=2):
    """The same DB and query count, ONE model with work (the next launch's grid shrinks) beside lists below MinPts."""
    return build_frame(N_A, Q_A, {37: (150, "blobs", 7), 3: (6, "tight", 8), 60: (2, "uniform", 9)}, seed=seed)


@functools.lru_cache(maxsize=None)
def no_match():
    return build_frame(N_A, Q_A, {}, seed=3)


@functools.lru_cache(maxsize=None)
def below_min_pts():
    return build_frame(N_A, Q_A, {m: (1 + j % 6, "tight", m) for j, m in enumerate(range(0, N_A, 3))}, seed=4)


def batch_e():
    """Four frames of one merged batch: no accepted match at all, case a, one busy model, only lists below MinPts."""
    return [no_match(), case_a(), one_busy(), below_min_pts()]


N_B, Q_B = 2500, 12000
NAMED_B = (0, 1023, 1024, 1025, 2047, 2048, 2499)


@functools.lru_cache(maxsize=None)
def case_b():
    """2 500 models: work on both sides of every 1024 boundary and in the last model, ~20 other models with work, ~300
    lists below MinPts, everything else empty."""
    rng = np.random.default_rng(0xB)
    spec = {}
    kinds = ("blobs", "tight", "chain", "uniform")
    for j, m in enumerate(NAMED_B):
        spec[m] = ((40, 8, 64, 7)[j % 4], ("blobs", "tight", "chain", "tight")[j % 4], 200 + j)
    rest = rng.permutation(np.setdiff1d(np.arange(N_B), NAMED_B))
    for j, m in enumerate(rest[:20]):
        spec[int(m)] = ((7, 8, 40, 64, 150)[j % 5], kinds[j % 4], 300 + j)
    for j, m in enumerate(rest[20:320]):
        spec[int(m)] = (1 + j % 6, kinds[j % 4], 400 + j)
    return build_frame(N_B, Q_B, spec, seed=5)


PRM_C = dict(radius=40.0, merge=20.0, min_pts=1, max_iter=100)
N_C = 12
SIZES_C = {0: 9, 2: 1, 3: 2, 4: 9, 5: 48, 7: 1, 9: 2, 11: 48}     # 3, 4, 5 next to each other; 11 = the DB's last model


@functools.lru_cache(maxsize=None)
def case_c():
    """n clusters in n points: every point of a 90-pixel grid is a cluster of its own, so a model's n + 1 start slots
    (cl_start + b + m) fill the region the next model's begin right behind."""
    return build_frame(N_C, 400, {m: (n, "grid90", 500 + m) for m, n in SIZES_C.items()}, seed=6)


N_D = 7
PRMS_D = {"iter1": dict(DEFAULT, max_iter=1), "iter2": dict(DEFAULT, max_iter=2), "iter100": DEFAULT,
          "r60": dict(radius=60.0, merge=20.0, min_pts=3, max_iter=100)}


@functools.lru_cache(maxsize=None)
def case_d():
    """uniform-400 with seeds 0..2 (the iteration cap changes their clusters), small lists on both sides of MinPts 3 / 7."""
    spec = {0: (400, "uniform", 0), 2: (400, "uniform", 1), 4: (400, "uniform", 2), 1: (7, "tight", 3), 3: (3, "tight", 4),
            5: (40, "blobs", 5), 6: (5, "tight", 6)}
    return build_frame(N_D, 2000, spec, seed=7)


N_F = 12
SHARED_F, EXACT_F = 4, 7       # the model whose images overlap; the model with a pair of MinPts and one of MinPts - 1


@functools.lru_cache(maxsize=None)
def case_f(n_images):
    """Several cameras: ~10 models whose matches spread over the images; model SHARED_F = blobs-60 with its points dealt
    to images 0 and 1 in turn (the same blobs in both: fewer clusters together than per image); model EXACT_F = a
    tight pair of exactly MinPts points in image 0 and one of MinPts - 1 in image 1."""
    rng = np.random.default_rng([0xF, n_images])
    spec = {}
    for j, m in enumerate((0, 1, 2, 3, 5, 6, 8, 9, 11)):
        n = (150, 40, 64, 8 * n_images, 400, 65, 30, 200, 90)[j]
        kind = ("blobs", "tight", "chain", "tight", "uniform", "blobs", "tight", "chain", "blobs")[j]
        spec[m] = (points(n, kind, 600 + m), rng.integers(0, n_images, n).astype(np.int32))
    spec[SHARED_F] = (points(60, "blobs", 0), (np.arange(60) % 2).astype(np.int32))
    mp = DEFAULT["min_pts"]
    spec[EXACT_F] = (points(2 * mp - 1, "tight", 77), np.array([0] * mp + [1] * (mp - 1), np.int32))
    return build_frame(N_F, 2500, spec, seed=8 + n_images, n_images=n_images)


N_G = 8


@functools.lru_cache(maxsize=None)
def case_g(n_clusters):
    """n_clusters tight-7 models: one cluster each."""
    return build_frame(N_G, 300, {m: (7, "tight", 700 + m) for m in range(n_clusters)}, seed=20 + n_clusters)


@functools.lru_cache(maxsize=None)
def case_g_over_cap():
    """A list of MS_CAP + 1 points beside an ordinary one."""
    return build_frame(N_G, 2600, {2: (MS_CAP + 1, "uniform", 9), 5: (40, "blobs", 10)}, seed=30)


@functools.lru_cache(maxsize=None)
def case_g_after_cap():
    return build_frame(N_G, 2600, {2: (MS_CAP, "uniform", 9), 5: (40, "blobs", 10)}, seed=31)
