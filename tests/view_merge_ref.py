"""The merge of re-seen points in numpy float32: what mh_view_merge_dev must write (the block above it in
include/moped_hip.h).  Built on view_model_ref.verdicts: `why == DUP` and dup["idx"] give each old row's observations,
in list order.

For an old row r of the model (rows [row_begin, row_end) of the store) with observations i_1 < .. < i_k, k >= 1:
    a = qn[i_1]; a = a + qn[i_j] (j = 2 .. k); if k > 1: a = a / float32(k);   s  = d_r * float32(c_r) + a
    b = X[i_1];  b = b + X[i_j]  (j = 2 .. k); if k > 1: b = b / float32(k);   p' = (p_r * float32(c_r) + b) / float32(c_r + 1)
Every operation is one float32 rounding, in the order written; the count becomes c_r + 1.  Rows with k = 0 are not
listed and keep their count."""
import numpy as np

import view_model_ref as ref

F = np.float32


def observations(why, dup_idx, row_begin, row_end):
    """-> {relative row: [keypoints, ascending]} for the keypoints rule 7 drops."""
    obs = {}
    for i in np.nonzero(np.asarray(why) == ref.DUP)[0]:
        r = int(dup_idx[i]) - row_begin
        assert 0 <= r < row_end - row_begin   # rule 7: the nearest row belongs to the model
        obs.setdefault(r, []).append(int(i))
    return obs


def fold(vectors, order=None):
    """The mean of the section above over `vectors` [k, n] float32 in the given order (default: as they lie)."""
    v = np.asarray(vectors, np.float32)
    order = range(len(v)) if order is None else order
    acc = None
    for j in order:
        acc = v[j].copy() if acc is None else acc + v[j]
    if len(v) > 1:
        acc = acc / F(len(v))
    assert acc.dtype == np.float32
    return acc


def merge(why, xyz, dup_idx, qn, old_desc, old_xyz, row_begin, row_end, views_in=None):
    """why, xyz: view_model_ref.verdicts' answer for the list; dup_idx: MATCH's nearest row per keypoint; qn [n,128] the
    descriptors as MATCH saw them; old_desc [N,128], old_xyz [N,3] the store as it holds them.
    -> (merged_idx [m] relative to row_begin, ascending; s [m,128] not normalised; p' [m,3]; views_out [rows])."""
    rows = row_end - row_begin
    views = np.ones(rows, np.int32) if views_in is None else np.array(views_in, np.int32)
    assert len(views) == rows and np.all(views >= 1)
    obs = observations(why, dup_idx, row_begin, row_end)
    qn = np.asarray(qn, np.float32)
    xyz = np.asarray(xyz, np.float32)
    idx = np.array(sorted(obs), np.int32)
    s = np.zeros((len(idx), 128), np.float32)
    p = np.zeros((len(idx), 3), np.float32)
    out = views.copy()
    with np.errstate(all="ignore"):
        for k, r in enumerate(idx):
            c = int(views[r])
            cf, c1 = F(c), F(c + 1)
            a = fold(qn[obs[r]])
            b = fold(xyz[obs[r]])
            s[k] = np.asarray(old_desc[row_begin + r], np.float32) * cf + a
            p[k] = (np.asarray(old_xyz[row_begin + r], np.float32) * cf + b) / c1
            out[r] = c + 1
    return idx, s, p, out


def merge_view(xy, n, depth, fill, pose, kw, dup, qn, old_desc, views_in=None):
    """The whole call for one list: verdicts under the spec `kw` (with merge_ratio / merge_dist) and the merge.
    dup: view_model_ref's dict + row_begin, row_end.  -> (why, xyz, merge(...))."""
    why, xyz = ref.verdicts(xy, n, depth, fill, pose, dup=dup, **{k: v for k, v in kw.items() if k != "max_rows"})
    return why, xyz, merge(why, xyz, dup["idx"], qn, old_desc, dup["xyz"], dup["row_begin"], dup["row_end"], views_in)
