"""moped3d's CLUSTER_WEIGHTED_MEAN_SHIFT_CPU (moped3d/libmoped/src/cluster/CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp:72-208)
restated in float32 numpy, operation for operation: what the device kernel (moped_amd/csrc/wms.hip) is tested against
where the recorded reference (tests/golden/wms_ref.npz, tests/tools/make_wms_golden.py) has no case.

Every sum over the points is np.add.accumulate over where(mask, term, 0): strictly in list order, as the reference adds.
Adding the +0 of a masked point changes nothing: a sum that starts at +0 never becomes -0 (round to nearest), and x + 0
is x for every other x, NaN included.  No shortcut is taken: the loop runs as long as the reference's does."""
import numpy as np

F = np.float32
CHUNK = 256   # canopies per block of the shift (bounds the [canopies, points, 3] intermediate)


def cauchy_weight(fill, hwd):
    """(float)(1.0 / (1.0 + (double)((d * d) / (g * g)))): the quotient in float, the rest in double (:184-186)."""
    d = np.asarray(fill, F)
    g = F(hwd)
    with np.errstate(all="ignore"):
        q = (d * d) / (g * g)
        return (1.0 / (1.0 + q.astype(np.float64))).astype(F)


def sq_dist(this, other):
    """Pt<3>::sqEuclDist: d = other[x] - this[x]; r += d * d over x = 0, 1, 2.  this [k, 3], other [n, 3] -> [k, n]."""
    with np.errstate(all="ignore"):
        r = np.zeros((len(this), len(other)), F)
        for x in range(3):
            d = other[None, :, x] - this[:, None, x]
            r = r + d * d
    return r


def weighted_mean_shift(xyz, weight, radius, merge, min_pts, max_iter):
    """WeighedMeanShift<3> (:72-158) -> (clusters, centre [n, 3], active [n], iterations); a cluster is an int32 array of
    positions in `xyz`, descending (push_front)."""
    P = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    w = np.ascontiguousarray(weight, F)
    n = len(P)
    if n == 0:
        return [], np.zeros((0, 3), F), np.zeros(0, bool), 0
    sq_radius, sq_merge = F(radius) * F(radius), F(merge) * F(merge)
    C = P.copy()
    active = np.ones(n, bool)
    PW = P * w[:, None]
    done, it = False, 0
    with np.errstate(all="ignore"):
        while not done and it < max_iter:
            done = True
            ids = np.flatnonzero(active)
            for c0 in range(0, len(ids), CHUNK):
                a = ids[c0:c0 + CHUNK]
                near = sq_dist(C[a], P) < sq_radius
                c = np.add.accumulate(np.where(near[:, :, None], PW[None], F(0)), axis=1)[:, -1]
                ws = np.add.accumulate(np.where(near, w[None], F(0)), axis=1)[:, -1]
                C[a] = c / ws[:, None]
            for a in ids:
                if not active[a] or a + 1 == n:
                    continue
                close = sq_dist(C[a:a + 1], C[a + 1:])[0] < sq_merge
                if close.any():
                    active[a + 1:][close] = False
                    done = False
            it += 1
    clusters = []
    for a in np.flatnonzero(active):
        mem = np.flatnonzero(sq_dist(C[a:a + 1], P)[0] < sq_radius)[::-1].astype(np.int32)
        if len(mem) > min_pts:
            clusters.append(mem)
    return clusters, C, active, it


def process(xyz, fill, image, images, radius, merge, min_pts, max_iter, hwd):
    """process() (:188-208) for one model -> (clusters of all images appended, [per image (positions, weight, centre,
    active, iterations)]); member indices are positions in that image's list."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    image = np.asarray(image)
    out, state = [], []
    for i in range(images):
        pos = np.flatnonzero(image == i)
        wt = cauchy_weight(np.asarray(fill, F)[pos], hwd)
        cl, C, act, it = weighted_mean_shift(xyz[pos], wt, radius, merge, min_pts, max_iter)
        out += cl
        state.append((pos, wt, C, act, it))
    return out, state


def same_floats(a, b):
    """Bit for bit, except that a NaN equals any NaN: its sign and payload are the processor's choice (x86 makes 0/0 a
    negative quiet NaN, gfx950 a positive one), not the algorithm's."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))
