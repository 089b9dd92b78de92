"""Cases for moped3d's depth front end -- DEPTHFILTER (features and per-model matches), DEPTHMAP_PROP and the
depth-adaptive ratio -- at the smallest map shapes that reach each edge of the device code (depth.hip, group.hip) and
of the reference's text (DEPTHFILTER_CPU.hpp).  Shared by tests/test_ref_steps_cpu.py (oracle == the reference's own
classes) and tests/test_gpu_depth_stages.py (device == oracle), so that the chain closes on the same inputs.

Shapes are (h, w, patch):
  (36, 100, 16)   ragged patch grid in x and in y
  (100, 36, 16)   portrait: the reference's `y1 = min((py+1)*PatchSize, width)` (:171) falls below y0 from the fourth
                  patch row on
  (37, 53, 8)     odd sizes
  (512, 512, 8)   4096 patches: feature_density_kernel's LDS arrays exactly full
  (480, 640, 64)  the workload's own
and (480, 640, 8) = 4800 patches, which the device must refuse.

Every map holds: depths of 0.4 .. 3 m that vary from patch to patch, a row of NaN depths, one patch of zero depth (what
invalid pixels are in real maps: area 0, an infinite density, a kept feature), one patch beyond MaximumDepth, one patch
wholly NaN (its minimum stays 1e10) and one negative pixel."""
import numpy as np

f32 = np.float32
SHAPES = ((36, 100, 16), (100, 36, 16), (37, 53, 8), (512, 512, 8), (480, 640, 64))
REFUSED_SHAPE = (480, 640, 8)
MAX_DEPTH, DEFAULT_DEPTH, CAUCHY_SCALE = 4.0, 1.0, 0.1
FILL_KINDS = ("none", "zeros", "mixed")
N_MODELS, ROWS_PER_MODEL = 3, 200


def intrinsics(h, w):
    return np.array([1.25 * w, 1.25 * w, w / 2, h / 2], f32)


def grid(h, w, patch):
    return -(-w // patch), -(-h // patch)      # pw, ph


def depth_map(h, w, patch, seed=0):
    """-> (img [h, w, 4] float32 = x, y, z, norm (norm -1 where the depth is unresolved), marks: the patch numbers of
    the planted regions)."""
    rng = np.random.default_rng([0xD3F7, h, w, patch, seed])
    pw, ph = grid(h, w, patch)
    base = rng.uniform(0.4, 2.8, size=(ph, pw))
    z = (np.kron(base, np.ones((patch, patch)))[:h, :w] + rng.uniform(0.0, 0.2, size=(h, w))).astype(f32)
    z[h // 2, :] = np.nan                                                     # the NaN band
    pick = rng.permutation(pw * ph)[:4]

    def block(p):
        py, px = divmod(int(p), pw)
        return slice(py * patch, min((py + 1) * patch, h)), slice(px * patch, min((px + 1) * patch, w))
    z[block(pick[0])] = np.nan
    z[block(pick[1])] = 0.0
    z[block(pick[2])] = 5.0
    ys, xs = block(pick[3])
    z[ys.start, xs.start] = -0.5
    K = intrinsics(h, w)
    v, u = np.mgrid[0:h, 0:w].astype(f32)
    img = np.zeros((h, w, 4), f32)
    with np.errstate(all="ignore"):
        img[..., 0] = (u - K[2]) / K[0] * z
        img[..., 1] = (v - K[3]) / K[1] * z
        img[..., 2] = z
        norm = np.sqrt((img[..., :3].astype(np.float64) ** 2).sum(-1)).astype(f32)
        img[..., 3] = np.where(z > 0, norm, f32(-1))
    return img, dict(all_nan=int(pick[0]), zero=int(pick[1]), far=int(pick[2]), negative=int(pick[3]))


def fill_map(h, w, kind, seed=0):
    """The distance map DEPTHMAP_PROP reads fillDistance from: None, zeros, or a mix of 0, exactly CauchyScale, small
    and large values (1e30: factor * factor overflows, the weight is 0)."""
    if kind == "none":
        return None
    if kind == "zeros":
        return np.zeros((h, w), f32)
    rng = np.random.default_rng([0xF111, h, w, seed])
    return rng.choice(np.array([0.0, CAUCHY_SCALE, 0.03, 0.25, 2.5, 1e6, 1e30], f32), size=(h, w)).astype(f32)


def coords(h, w, patch, n, seed=0, outside=False, aim=()):
    """n image coordinates (float32 [n, 2]): fractional ones all over the map, a good third of them crowded into three
    patches (so that densities differ), coordinates exactly on patch boundaries and the float just below, w - 0.01 and
    h - 0.01, duplicates.  outside: also coordinates off the map (-0.5, -3.2, >= w, >= h), where the reference reads out
    of bounds and device and oracle clamp.  aim: patch numbers that get three points each (the planted regions of
    depth_map, which coordinates drawn all over a large map would miss)."""
    rng = np.random.default_rng([0xC00D, h, w, patch, seed])
    pw, ph = grid(h, w, patch)
    special = []
    for k in rng.permutation(np.arange(1, pw))[:6]:
        y = rng.uniform(0, h)
        special += [(k * patch, y), (np.nextafter(f32(k * patch), f32(0)), y)]
    for k in rng.permutation(np.arange(1, ph))[:6]:
        x = rng.uniform(0, w)
        special += [(x, k * patch), (x, np.nextafter(f32(k * patch), f32(0)))]
    special += [(w - 0.01, rng.uniform(0, h)), (rng.uniform(0, w), h - 0.01), (w - 0.01, h - 0.01), (0.0, 0.0)]
    if outside:
        special += [(-0.5, rng.uniform(0, h)), (-3.2, rng.uniform(0, h)), (w, rng.uniform(0, h)), (w + 7.3, rng.uniform(0, h)),
                    (rng.uniform(0, w), -0.5), (rng.uniform(0, w), -3.2), (rng.uniform(0, w), h), (rng.uniform(0, w), h + 2.5),
                    (-1.0, -1.0), (w, h)]
    for p in aim:
        py, px = divmod(int(p), pw)
        x0, y0, x1, y1 = px * patch, py * patch, min((px + 1) * patch, w), min((py + 1) * patch, h)
        special += [(x0, y0)] + [tuple(q) for q in rng.uniform([x0, y0], [x1, y1], size=(2, 2))]
    special = np.array(special, np.float64)
    n_dup = max(2, n // 20)
    n_rand = n - len(special) - n_dup
    assert n_rand > 10
    n_crowd = n_rand * 2 // 5
    pts = [rng.uniform([0, 0], [w, h], size=(n_rand - n_crowd, 2))]
    for p in rng.permutation(pw * ph)[:3]:
        py, px = divmod(int(p), pw)
        x0, y0, x1, y1 = px * patch, py * patch, min((px + 1) * patch, w), min((py + 1) * patch, h)
        k = n_crowd // 3 if len(pts) < 3 else n_crowd - 2 * (n_crowd // 3)
        pts.append(rng.uniform([x0, y0], [x1, y1], size=(k, 2)))
    uv = np.concatenate(pts + [special])
    uv = np.concatenate([uv, uv[rng.integers(0, len(uv), n_dup)]])
    uv = uv[rng.permutation(len(uv))].astype(f32)
    if not outside:      # float32 rounding of a coordinate just below w must not reach w
        uv[:, 0] = np.clip(uv[:, 0], 0, np.nextafter(f32(w), f32(0)))
        uv[:, 1] = np.clip(uv[:, 1], 0, np.nextafter(f32(h), f32(0)))
    assert len(uv) == n
    return uv


def groups(n, seed=0, n_models=N_MODELS):
    """Offsets that split n points into n_models consecutive groups of uneven sizes (the per-model match lists)."""
    rng = np.random.default_rng([0x6209, n, seed])
    cuts = np.sort(rng.integers(0, n + 1, n_models - 1))
    return np.concatenate([[0], cuts, [n]]).astype(np.int32)


def tie_density(value):
    """A Density whose `Density*100*100` (Float operations, DEPTHFILTER_CPU.hpp:130) equals `value` bit for bit, searched
    40 ulp either side of value / 1e4; None where there is none."""
    import orclib
    value = f32(value)
    if not np.isfinite(value) or value <= 0:
        return None
    d0 = f32(np.float64(value) / 1e4)
    bits = int(d0.view(np.uint32))
    for k in sorted(range(-40, 41), key=abs):
        d = np.uint32(bits + k).view(f32)
        if orclib.density_filter(d) == value:
            return float(d)
    return None


# ---- frames for the device: a small DB, queries that are DB rows with noise -----------------------------------------
def make_db(seed=0xDE7):
    from moped_amd import synth
    return synth.make_db(N_MODELS, ROWS_PER_MODEL, seed=seed)


def queries(db, Q, seed=0, sigma=0.004):
    """Q query descriptors = DB rows + N(0, sigma^2) per dimension (sigma a scalar, or (lo, hi): drawn per query, so that
    d1 / d2 spreads over the ratio test's range) -> (desc [Q, 128], row [Q])."""
    rng = np.random.default_rng([0x9E27, Q, seed])
    row = rng.integers(0, db.n, Q)
    s = np.full(Q, sigma, np.float64) if np.isscalar(sigma) else rng.uniform(sigma[0], sigma[1], Q)
    d = db.desc[row] + rng.normal(0, 1, size=(Q, 128)) * s[:, None]
    return np.ascontiguousarray(np.maximum(d, 0), f32), row
