"""References for the linkage clusterer's two halves (moped3d/libmoped/src/cluster/CLUSTER_LINKAGE_CPU.hpp; line numbers
below are that file's), independent of oracle/linkage_oracle.cpp and of the kernel:

  agglomerate      hierarchicalCluster (:416-540) written down a second time, in Python, over a given similarity matrix --
                   list handling, all three linkage types -- with counts of what the list handling did (stale merges,
                   skipped first indices), so that a test can assert its input still exercises them.
  similarity_f64   the matrix stages (:97-366) in float64: what the float32 chain of oracle and device approximates.
                   The Bresenham walk (:176-220) stays in float32 exactly as written -- every operation in it is
                   correctly rounded, so oracle, device and this file visit the same pixels; only values are float64.

Inputs are generated here too (lattice, flat map): nothing in this file needs a GPU."""
import numpy as np

F = np.float32
W, H = 640, 480


def agglomerate(Km, cutoff, min_pts, ltype):
    """-> (clusters with more than min_pts members as lists, stats).  The absorbed cluster's index stays in the list of
    live indices until the NEXT scan reaches it as a first index (:446-463: erased there, and the element behind it is
    skipped as a first index of that scan), so earlier first indices still pair with it through the row the last update
    left it -- a merge won that way absorbs an EMPTY cluster ("stale").  Update of row `first` after a merge:
      1 (average, :515-523)  float((1.0 / (S1 + S2)) * double(float(S1) * d1 + float(S2) * d2)), products and sum float32
      0 / 2 (:380-413, 525)  minimum / maximum of K over the pairs of the two clusters, by `<` / `>` from 1e20 / -1 (NaN
                             never wins; an empty cluster leaves the start value)."""
    Km = np.asarray(Km, F)
    n = len(Km)
    cutoff = F(cutoff)
    cl = [[i] for i in range(n)]
    live = list(range(n))
    D = Km.copy()
    stats = dict(merges=0, stale=0, skipped=0)

    def link(a, b):
        v = Km[np.ix_(b, a)].ravel() if a and b else np.zeros(0, F)
        v = v[~np.isnan(v)]
        if ltype == 0:
            return min(F(1e20), v.min()) if len(v) else F(1e20)
        return max(F(-1), v.max()) if len(v) else F(-1)

    remove = -1
    while True:
        best, pair = F(-1), (0, 0)
        x = 0
        while x < len(live):
            i = live[x]
            if i == remove:
                del live[x]          # erase; the loop's increment then skips the element that moved into this place
                stats["skipped"] += x < len(live)
                x += 1
                continue
            js = live[x + 1:]
            if js:
                v = D[i, js]
                v = np.where(np.isnan(v), -np.inf, v)
                k = int(np.argmax(v))                     # the first maximum of the row ...
                if v[k] > best:                           # ... wins only if it beats the rows before it
                    best, pair = v[k], (i, js[k])
            x += 1
        if best < cutoff:
            break
        i, j = pair
        s1, s2 = len(cl[i]), len(cl[j])
        stats["merges"] += 1
        stats["stale"] += s2 == 0
        cl[i] += cl[j][::-1]
        cl[j] = []
        remove = j
        if ltype == 1:
            with np.errstate(all="ignore"):
                row = (F(s1) * D[i] + F(s2) * D[j]).astype(F)            # float32 products, float32 sum
                row = ((1.0 / (s1 + s2)) * row.astype(np.float64)).astype(F)
        else:
            row = np.array([link(cl[k], cl[i]) for k in range(n)], F)
        D[i, :] = row
        D[:, i] = row
    return [c for c in cl if len(c) > min_pts], stats


# ---- inputs ---------------------------------------------------------------------------------------------------------

def flat_map(z=1.0, K=(800.0, 800.0, 320.0, 240.0)):
    """[H, W, 4] depth map (x, y, z, norm) of a plane at depth z."""
    v, u = np.mgrid[0:H, 0:W].astype(F)
    img = np.zeros((H, W, 4), F)
    img[..., 0] = (u - F(K[2])) / F(K[0]) * F(z)
    img[..., 1] = (v - F(K[3])) / F(K[1]) * F(z)
    img[..., 2] = z
    img[..., 3] = np.sqrt((img[..., :3] ** 2).sum(-1))
    return img


def lattice(n, step=12, x0=100.5, y0=80.5):
    """n points of a square pixel lattice, row by row (6 x 6 for n = 36): few distinct similarities, every merge a tie."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return np.stack([x0 + step * (k % side), y0 + step * (k // side)], 1).astype(F)


def world_of(img, uv):
    """Camera-frame points of the pixels the image points truncate to (what DEPTHMAP_PROP hands the clusterer)."""
    x = np.clip(uv[:, 0].astype(np.int32), 0, img.shape[1] - 1)
    y = np.clip(uv[:, 1].astype(np.int32), 0, img.shape[0] - 1)
    return np.ascontiguousarray(img[y, x, :3], F)


# ---- the matrix stages in float64 ----------------------------------------------------------------------------------------

def _walk_max_angle(img, px, py, qx, qy):
    """getDiscontinuityMatrix's maxAngleDiff (:244-283) for pairs of pixels (int arrays), float64 values over the float32
    Bresenham walk of bresenhamIterate (:176-220)."""
    h, w = img.shape[:2]
    z = img[..., 2].astype(np.float64)
    direct = np.arctan2(z[qy, qx] - z[py, px], np.sqrt(((px - qx) ** 2 + (py - qy) ** 2).astype(np.float64)))
    x0, y0, x1, y1 = px.copy(), py.copy(), qx.copy(), qy.copy()
    steep = np.abs(y1 - y0) > np.abs(x1 - x0)
    x0, y0 = np.where(steep, y0, x0), np.where(steep, x0, y0)
    x1, y1 = np.where(steep, y1, x1), np.where(steep, x1, y1)
    sw = x0 > x1
    x0, x1 = np.where(sw, x1, x0), np.where(sw, x0, x1)
    y0, y1 = np.where(sw, y1, y0), np.where(sw, y0, y1)
    with np.errstate(all="ignore"):
        delta_x = x1.astype(F) - x0.astype(F)
        delta_y = np.abs(y1.astype(F) - y0.astype(F))
        y_step = np.where(y0 < y1, 1, -1).astype(F)
        per = np.maximum((x1 - x0) // 20, 1)
        d_err = delta_y / delta_x                                   # (0 / 0 when p == q: never used, one sample)
        inc = (d_err * per.astype(F)) * y_step                      # float32: deltaError * perStep * yStep
    err = np.zeros(len(px), F)
    x, y = x0.copy(), y0.copy()
    best = np.full(len(px), -1.0)
    act = np.ones(len(px), bool)
    pax = pay = None
    while act.any():
        cx, cy = np.where(steep, y, x), np.where(steep, x, y)
        if pax is not None:
            a = np.nonzero(act)[0]
            ax, ay = np.clip(pax[a], 0, w - 1), np.clip(pay[a], 0, h - 1)
            bx, by = np.clip(cx[a], 0, w - 1), np.clip(cy[a], 0, h - 1)
            dist = np.sqrt(((pax[a] - cx[a]) ** 2 + (pay[a] - cy[a]) ** 2).astype(np.float64))
            with np.errstate(all="ignore"):
                diff = np.abs(direct[a] - np.arctan2(z[by, bx] - z[ay, ax], dist))
                best[a] = np.where(diff > best[a], diff, best[a])   # `if (angleDiff > maxAngleDiff)`: NaN never wins
        pax, pay = cx, cy
        x = x + per
        act = act & (x <= x1)
        a = np.nonzero(act)[0]
        with np.errstate(all="ignore"):
            frac, whole = np.modf((err[a] + inc[a]).astype(F))
        err[a] = frac
        y[a] = (y[a].astype(F) + whole).astype(np.int64)            # y += intPart
    return best


def _max_from_minus_one(M):
    """normalizeSimilarityMatrix's maximum (:306-313): `if (v > max)` from -1, so NaN never wins."""
    v = M[~np.isnan(M)]
    return max(-1.0, v.max()) if v.size else -1.0


def similarity_f64(uv, model_xyz, world_xyz, img, fill, use3d_filter=2, sigma2d=-1.0, sigma3d=-1.0):
    """-> (A, K) float64 [n, n]: A = K3D + discontinuity kernel, normalised, + / x K3F, before its last normalisation (with
    use3d_filter 0: the first sum, not normalised); K = the fill-weighted sum of K2D and the normalised A (:325-366).
    Constants the source states as Float (sigma 0.1, gamma 25, pi/128's square) are taken as the float32 values."""
    n = len(uv)
    uv64, mx, wx = (np.asarray(a, F).astype(np.float64) for a in (uv, model_xyz, world_xyz))
    h, w = img.shape[:2]
    with np.errstate(all="ignore"):
        d2 = ((uv64[:, None] - uv64[None]) ** 2).sum(-1)
        dm = np.sqrt(((mx[:, None] - mx[None]) ** 2).sum(-1))
        dw2 = ((wx[:, None] - wx[None]) ** 2).sum(-1)
        # sigmas: getAverageNNDistances (:97-123); a single point has no neighbour (DBL_MAX as Float = inf)
        s2, s3 = float(F(sigma2d)), float(F(sigma3d))
        if sigma2d == -1 or sigma3d == -1:
            nn2, nn3 = np.sqrt(d2), dm.copy()
            np.fill_diagonal(nn2, np.inf)
            np.fill_diagonal(nn3, np.inf)
            # `if (nn > d)` from inf: NaN distances never become the minimum
            a2 = np.where(np.isnan(nn2), np.inf, nn2).min(1).sum() / n
            a3 = np.where(np.isnan(nn3), np.inf, nn3).min(1).sum() / n
            if sigma2d == -1:
                s2 = a2
            if sigma3d == -1:
                s3 = a3
        K2D = np.exp(-d2 / (2 * s2 * s2))
        K3D = np.exp(-dw2 / (2 * s3 * s3))
        # discontinuity kernel (:231-285), pairs i <= j, mirrored
        px = np.clip(np.asarray(uv, F)[:, 0].astype(np.int64), 0, w - 1)
        py = np.clip(np.asarray(uv, F)[:, 1].astype(np.int64), 0, h - 1)
        i, j = np.triu_indices(n)
        ang = _walk_max_angle(img, px[i], py[i], px[j], py[j])
        bk = np.zeros((n, n))
        bk[i, j] = bk[j, i] = np.exp(ang * ang / float(F(-2 * (np.pi / 128) * (np.pi / 128))))
        A = K3D + bk
        if use3d_filter:
            A = A / _max_from_minus_one(A)
            dr = np.sqrt(dw2)
            de = np.abs(dm - dr) / dm
            sg = float(F(0.1))
            k3f = np.exp(-de * de / float(F(2 * sg * sg)))
            np.fill_diagonal(k3f, 1.0)
            A = A + k3f if use3d_filter == 1 else A * k3f
        K3 = A / _max_from_minus_one(A)
        if fill is None:
            wgt = np.ones(n)
        else:
            d = np.asarray(fill, F)[py, px].astype(np.float64)
            wgt = 1.0 / (1.0 + d * d / 625.0)
        jw = wgt[:, None] * wgt[None]
        K = (0.5 + 0.5 * (1.0 - jw)) * K2D + (0.5 * jw) * K3
    return A, K
