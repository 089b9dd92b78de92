"""getConvexHull (moped2/libmoped/include/moped.hpp:293-327) restated in float32, for the tests of the object hulls.

chain(points): the sort by Pt<2>::operator< (x, then y) and the monotone chain as the reference runs it -- forward to
the last point, back to the first, popping while det <= 0, the determinant
    det = (p0x - p1x) * (p2y - p1y) - (p2x - p1x) * (p0y - p1y)          (p2 the newest point)
with every operation rounded to float32 on its own (no fused multiply-add).  Each operation is done in double and then
rounded: for + - * of float32 operands that is the correctly rounded float32 result (53 >= 2 * 24 + 2 bits), and it is
what keeps a 5 000-point cloud at a few milliseconds.  The vertex order is the reference's: the backward half, newest
point first, without the first point; then the forward half, newest first, without the last point.  1 point -> empty,
2 points -> both, 0 points (undefined in the reference) -> empty.

prefilter(points): the eight-direction extreme-point prefilter of csrc/hull.hip in float32 -- what is strictly left of
every edge (that has a length) of the octagon of the extremes, by more than 1e-4 * span^2, is discarded.
chain_prefiltered = chain(prefilter(points)).

object_hull(...): project (orclib.project = the oracle's project()), leave out what project() marks as behind the
camera (FLT_MAX, FLT_MAX) -- the device's documented departure -- and chain the rest.  bbox_corners: the projected corners
of the model's bounding box in the order [x][y][z] of GLOBAL_DISPLAY.hpp:198-203."""
import struct

import numpy as np

FLT_MAX = np.float32(3.402823466e+38)
_pack, _unpack = struct.Struct("f").pack, struct.Struct("f").unpack


def _r(x):
    """A double rounded to float32 (overflow -> inf, as the hardware rounds)."""
    try:
        return _unpack(_pack(x))[0]
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


def _det(p0, p1, p2):
    return _r(_r(_r(p0[0] - p1[0]) * _r(p2[1] - p1[1])) - _r(_r(p2[0] - p1[0]) * _r(p0[1] - p1[1])))


def sort_points(points):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def _half(seq):
    """One direction of the chain over the points of seq: the stack, oldest first."""
    st = []
    for q in seq:
        while len(st) >= 2 and _det(st[-2], st[-1], q) <= 0:
            st.pop()
        st.append(q)
    return st


def chain(points):
    p = sort_points(points)
    n = len(p)
    if n < 2:
        return np.zeros((0, 2), np.float32)
    pts = [(float(x), float(y)) for x, y in p]
    fwd = _half(pts)            # pts[0] ... pts[n - 1]
    bwd = _half(pts[::-1])      # pts[n - 1] ... pts[0]
    out = bwd[-2::-1] + fwd[-2::-1]
    return np.array(out, np.float32).reshape(-1, 2)


def prefilter(points):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    if len(p) == 0:
        return p
    x, y = p[:, 0], p[:, 1]
    keys = [x, x + y, y, y - x, -x, -(x + y), -y, x - y]   # counter-clockwise
    ext = p[[int(np.argmax(k)) for k in keys]]
    d = np.roll(ext, -1, axis=0) - ext
    live = (d[:, 0] != 0) | (d[:, 1] != 0)
    span = max(ext[0, 0] - ext[4, 0], ext[2, 1] - ext[6, 1])
    margin = np.float32(1e-4) * span * span
    if not live.any() or not np.isfinite(margin):
        return p
    inside = np.ones(len(p), bool)
    with np.errstate(all="ignore"):
        for e in np.nonzero(live)[0]:
            cr = d[e, 0] * (y - ext[e, 1]) - d[e, 1] * (x - ext[e, 0])
            inside &= cr > margin
    return p[~inside]


def chain_prefiltered(points):
    return chain(prefilter(points))


def same_vertices(a, b):
    """Equal as VALUES (so -0.0 == 0.0: std::sort may return either of two equal points)."""
    a = np.asarray(a, np.float32).reshape(-1, 2)
    b = np.asarray(b, np.float32).reshape(-1, 2)
    return a.shape == b.shape and bool(np.all(a == b))


def project_front(pose7, xyz, K, cam):
    """(the projected points in front of the camera, n_behind)"""
    import orclib
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros((0, 2), np.float32), 0
    uv = orclib.project(pose7, xyz, K, cam)
    behind = (uv[:, 0] == FLT_MAX) & (uv[:, 1] == FLT_MAX)
    return uv[~behind], int(behind.sum())


def object_hull(pose7, xyz, K, cam, prefiltered=False):
    """-> (hull [k, 2], n_behind)"""
    uv, n_behind = project_front(pose7, xyz, K, cam)
    return (chain_prefiltered if prefiltered else chain)(uv), n_behind


def bbox_corners(pose7, xyz, K, cam):
    import orclib
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz):
        box = np.stack([xyz.min(0), xyz.max(0)])
    else:
        box = np.array([[10E10] * 3, [-10E10] * 3], np.float32)   # moped.cpp:107-108
    c = np.array([[box[ix, 0], box[iy, 1], box[iz, 2]] for ix in (0, 1) for iy in (0, 1) for iz in (0, 1)], np.float32)
    return orclib.project(pose7, c, K, cam)
