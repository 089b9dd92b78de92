"""The row-maxima form of hierarchicalCluster (moped3d/libmoped/src/cluster/CLUSTER_LINKAGE_CPU.hpp:416-540) in numpy:
the rules moped_amd/csrc/linkage_rowmax.hip runs (MH_LINKAGE_ROWMAX), written down on the CPU so that they can be held
against the oracle's plain restatement of the reference (orclib.linkage_agglomerate) without a GPU.

For every listed row a: cache[a] = (value, column), the first maximum of D[a, b] over the listed columns b > a -- strict
`>` from -1, ties to the smaller column, NaN never wins.  A scan is the first maximum of the caches in ascending a.
  - The scan after a merge (first, second): removeValue = second is still listed as a column; rows removeValue and `skip`
    (the next listed index after removeValue; only if removeValue was still listed) are left out of the reduction only.
  - When that scan ends removeValue is delisted: listed rows a < removeValue with cached column removeValue are dirty.
  - The merge rewrites D[first, i] = D[i, first] = nv[i]: row `first` is dirty; a listed row a < first with cached column
    `first` keeps it with the new value when nv[a] >= the cached value, else (smaller or NaN) it is dirty; with another
    cached column it takes (nv[a], first) when nv[a] > the cached value, or equal with first < the cached column.
  - Dirty rows that are still listed are rescanned before the next scan.
  - A stale winner (a, removeValue) is a merge with S2 = 0.
The row update for minimum / maximum linkage is the kernel's: the minimum (maximum) of the two rows' entries, which hold
the two clusters' minima (maxima); 1e20 / -1 for an emptied cluster and where only NaN is left."""
import numpy as np

F = np.float32
NONE = -1


def _rescan(D, listed, a):
    """-> (value, column) of row a over the listed columns b > a."""
    cols = np.nonzero(listed[a + 1:])[0] + a + 1
    if len(cols) == 0:
        return F(-1), NONE
    v = D[a, cols]
    v = np.where(np.isnan(v), -np.inf, v)
    k = int(np.argmax(v))                   # first maximum
    if not v[k] > -1:
        return F(-1), NONE
    return F(v[k]), int(cols[k])


def agglomerate_rowmax(Km, cutoff, min_pts, ltype):
    """-> (clusters with more than min_pts members as lists in the reference's member order, stats)."""
    D = np.array(Km, F)
    n = len(D)
    cutoff = F(cutoff)
    cl = [[i] for i in range(n)]
    size = np.ones(n, np.int64)
    listed = np.ones(n, bool)
    cv = np.full(n, -1, F)
    cc = np.full(n, NONE, np.int64)
    for a in range(n):
        cv[a], cc[a] = _rescan(D, listed, a)
    stats = dict(merges=0, stale=0, rescans=0)
    remove = -1
    for _ in range(2 * n + 2):
        rv_listed = remove >= 0 and listed[remove]
        skip = -1
        if rv_listed:
            later = np.nonzero(listed[remove + 1:])[0]
            if len(later):
                skip = remove + 1 + int(later[0])
        rows = listed & (cc != NONE)
        if remove >= 0:
            rows[remove] = False
        if skip >= 0:
            rows[skip] = False
        best, first = F(-1), -1
        if rows.any():
            v = np.where(rows, cv, -np.inf)         # (a cached value is never NaN: NaN never wins a row)
            k = int(np.argmax(v))                   # first maximum in ascending a
            if v[k] > -1:
                best, first = F(v[k]), k
        dirty = set()
        if rv_listed:
            listed[remove] = False
            dirty |= {a for a in range(remove) if listed[a] and cc[a] == remove}
        if best < cutoff or first < 0:
            break
        second = int(cc[first])
        s1, s2 = int(size[first]), int(size[second])
        stats["merges"] += 1
        stats["stale"] += s2 == 0
        cl[first] += cl[second][::-1]
        cl[second] = []
        da, db = D[first].copy(), D[second].copy()
        with np.errstate(all="ignore"):
            if ltype == 1:
                nv = (F(s1) * da + F(s2) * db).astype(F)
                nv = ((1.0 / (s1 + s2)) * nv.astype(np.float64)).astype(F)
            else:
                start = F(1e20) if ltype == 0 else F(-1)
                both = np.fmin(da, db) if ltype == 0 else np.fmax(da, db)
                nv = da.copy() if s2 == 0 else both
                empty = size == 0
                empty[second] = True
                nv[empty] = start
                nv[np.isnan(nv)] = start
                nv = nv.astype(F)
        size[first] = s1 + s2
        size[second] = 0
        D[first, :] = nv
        D[:, first] = nv
        dirty.add(first)
        clean = listed[:first].copy()
        clean[[a for a in dirty if a < first]] = False
        x, v, c = nv[:first], cv[:first], cc[:first]           # (views: the caches are updated in place)
        with np.errstate(invalid="ignore"):
            same = clean & (c == first)
            keep = same & (x >= v)
            take = clean & ~same & ((x > v) | ((x == v) & (c != NONE) & (first < c)))
        dirty |= set(np.nonzero(same & ~keep)[0].tolist())
        v[keep] = x[keep]
        v[take] = x[take]
        c[take] = first
        for a in dirty:
            if listed[a]:
                cv[a], cc[a] = _rescan(D, listed, a)
                stats["rescans"] += 1
        remove = second
    return [c for c in cl if len(c) > min_pts], stats
