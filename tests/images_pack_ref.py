"""numpy restatement of the hand-over from FEAT's per-image lists to the packed lists of frames with several cameras
(moped_amd/csrc/images_pack.hip; FEAT_SIFT_CPU.hpp:80-107 appends image 0's keypoints, then image 1's, ..., imageIdx = i).

FEAT leaves image j = f * n_images + i of a batch at rows [j * cap, (j + 1) * cap) of a staging area with its count in
counts[j] (which may exceed cap).  Frame f's packed list starts at row f * n_images * cap of the frame buffers and holds
the first min(counts[j], cap) rows of its image 0, then of its image 1, ...; rows past the frame's total are not written.
"""
import numpy as np


def layout(counts, cap, n_images):
    """counts [F * n_images] -> (clamped [F, n_images], totals [F], rows): rows[f] = (image [total], source row [total])
    of every packed row of frame f, the source row counted in the staging area (j * cap + k)."""
    counts = np.asarray(counts, np.int64).reshape(-1, n_images)
    clamped = np.clip(counts, 0, cap)
    totals = clamped.sum(1)
    rows = []
    for f, cl in enumerate(clamped):
        img = np.repeat(np.arange(n_images), cl)
        first = np.concatenate([[0], np.cumsum(cl)[:-1]])          # exclusive scan: first packed row of every image
        k = np.arange(int(cl.sum())) - first[img]
        rows.append((img.astype(np.int32), ((f * n_images + img) * cap + k).astype(np.int64)))
    return clamped.astype(np.int32), totals.astype(np.int32), rows


def pack(stage_desc, stage_xy, counts, cap, n_images, fill=np.nan):
    """The frame buffers after the hand-over: desc [F * n_images * cap, 128], xy [.., 2], image [..] (int32), rows that
    are not written = `fill` (-1 for the image index), + (clamped, totals)."""
    clamped, totals, rows = layout(counts, cap, n_images)
    F = len(totals)
    Q = n_images * cap
    desc = np.full((F * Q, stage_desc.shape[1]), fill, np.float32)
    xy = np.full((F * Q, 2), fill, np.float32)
    image = np.full(F * Q, -1, np.int32)
    for f, (img, src) in enumerate(rows):
        n = len(img)
        desc[f * Q:f * Q + n] = stage_desc[src]
        xy[f * Q:f * Q + n] = stage_xy[src]
        image[f * Q:f * Q + n] = img
    return desc, xy, image, clamped, totals


def pack_lists(lists, cap, n_images):
    """lists = [(desc [c, 128], xy [c, 2])] of F * n_images images in list order -> per frame (desc, xy, image, clamped
    counts): the packed list as the host would build it knowing the counts."""
    out = []
    for f in range(len(lists) // n_images):
        mine = lists[f * n_images:(f + 1) * n_images]
        cl = [min(len(d), cap) for d, _ in mine]
        desc = np.concatenate([np.asarray(d, np.float32)[:c].reshape(-1, 128) for (d, _), c in zip(mine, cl)])
        xy = np.concatenate([np.asarray(x, np.float32)[:c].reshape(-1, 2) for (_, x), c in zip(mine, cl)])
        image = np.repeat(np.arange(n_images, dtype=np.int32), cl)
        out.append((desc, xy, image, np.array(cl, np.int32)))
    return out
