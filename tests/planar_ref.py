"""Planar models from a keypoint list, in numpy: what mh_planar_rows_dev must write and what mh_models_write_xml must
print (Moped::createPlanarModelsFromImages, moped2/libmoped/src/moped.cpp:196-236; sXML::print, include/sXML.hpp:146-170;
toString, include/moped.hpp:359-360).

Selection: keypoint i < min(n, cap) is kept if roi[0] <= u < roi[2] and roi[1] <= v < roi[3] on the float32
coordinates (a NaN fails every comparison); roi None or all zeros keeps every keypoint; only the first max_rows kept ones
(and the first out_cap) are written, in list order.  Coordinates: one float32 rounding per operation."""
import numpy as np

BIG = np.float32(10E10)   # moped.cpp:107-108


def keep_mask(xy, n, roi=None):
    xy = np.asarray(xy, np.float32)
    n = max(0, min(int(n), len(xy)))
    keep = np.zeros(len(xy), bool)
    if roi is None or not np.any(np.asarray(roi, np.float32)):
        keep[:n] = True
        return keep
    r = np.asarray(roi, np.float32)
    u, v = xy[:n, 0], xy[:n, 1]
    with np.errstate(invalid="ignore"):
        keep[:n] = (u >= r[0]) & (u < r[2]) & (v >= r[1]) & (v < r[3])
    return keep


def coords(xy, form, scale=1.0, K=(1, 1, 0, 0), z=0.0):
    """[n,3] float32: form 0 (u scale, v scale, 0); form 1 ((u - cx) / fx z, (v - cy) / fy z, z)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    u, v = xy[:, 0], xy[:, 1]
    f = np.float32
    with np.errstate(all="ignore"):
        if form == 0:
            x, y, zz = u * f(scale), v * f(scale), np.zeros(len(u), np.float32)
        else:
            fx, fy, cx, cy = (f(k) for k in K)
            x = ((u - cx) / fx) * f(z)
            y = ((v - cy) / fy) * f(z)
            zz = np.full(len(u), f(z), np.float32)
    out = np.stack([x, y, zz], 1)
    assert out.dtype == np.float32
    return out


def bbox(xyz):
    """Model::boundingBox: min xyz, max xyz from +-10E10 by `<` and `>` (a NaN leaves it as it is)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    lo, hi = np.full(3, BIG, np.float32), np.full(3, -BIG, np.float32)
    for k in range(3 if len(xyz) else 0):
        col = xyz[:, k]
        # `if (v < lo) lo = v` row after row: the FIRST row that holds the extreme value (so +0 before -0 stays +0)
        below = np.nonzero(np.where(np.isnan(col), BIG, col) < BIG)[0]
        if len(below):
            lo[k] = col[below[np.argmin(col[below])]]
        above = np.nonzero(np.where(np.isnan(col), -BIG, col) > -BIG)[0]
        if len(above):
            hi[k] = col[above[np.argmax(col[above])]]
    return np.concatenate([lo, hi]).astype(np.float32)


def rows(desc, xy, n, form, scale=1.0, K=(1, 1, 0, 0), z=0.0, roi=None, max_rows=0, out_cap=None):
    """-> (desc [k,128], xyz [k,3], bbox [6], kept indices)."""
    desc = np.asarray(desc, np.float32).reshape(-1, 128)
    idx = np.nonzero(keep_mask(xy, n, roi))[0]
    if max_rows > 0:
        idx = idx[:max_rows]
    if out_cap is not None:
        idx = idx[:out_cap]
    xyz = coords(np.asarray(xy, np.float32)[idx], form, scale, K, z)
    return desc[idx].copy(), xyz, bbox(xyz), idx


def g(v):
    """toString(float): ostream << float = %g with 6 significant digits."""
    return "%g" % float(np.float32(v))


def xml_text(name, desc, xyz, desc_type="SIFT"):
    desc = np.asarray(desc, np.float32).reshape(-1, 128)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = ['<Model name="%s">\n' % name]
    if len(desc) == 0:
        out.append("\t<Points/>\n")
    else:
        out.append("\t<Points>\n")
        for d, p in zip(desc, xyz):   # properties in std::map order: desc, desc_type, p3d
            out.append('\t\t<Point desc="%s" desc_type="%s" p3d="%s"/>\n'
                       % (" ".join(g(x) for x in d), desc_type, " ".join(g(x) for x in p)))
        out.append("\t</Points>\n")
    out.append("</Model>\n")
    return "".join(out)


def round6(a):
    """The float32 values a reader gets back from the 6-digit text."""
    a = np.asarray(a, np.float32)
    return np.array([np.float32(g(x)) for x in a.reshape(-1)], np.float32).reshape(a.shape)


def form1_cases():
    """Keypoints and (K, z) for which form 1 with the division by fx replaced by a multiplication with fl(1 / fx)
    differs in the last bit of x.  That reciprocal-multiply is the rewrite a fast-math build makes, and the real
    discriminator: (u - cx) / fx z has no multiply followed by an add, so a fused multiply-add has nothing to contract
    unless the division has been rewritten first.  Checked here on the CPU: every returned keypoint separates the two."""
    f = np.float32
    K = (f(525.0), f(519.0), f(319.5), f(239.5))
    z = f(0.8)
    rng = np.random.default_rng(0x9A7)
    uv = rng.uniform(0, 640, (8192, 2)).astype(np.float32)
    u = uv[:, 0]
    exact = ((u - K[2]) / K[0]) * z
    recip = ((u - K[2]) * (f(1) / K[0])) * z
    sep = np.nonzero(exact.view(np.uint32) != recip.view(np.uint32))[0]
    assert len(sep) >= 32, "no value separates a division from a reciprocal multiply"
    return uv[sep[:64]].copy(), K, z


def form0_cases():
    """Keypoints and a scale = fl(0.8 / 525) whose products fl(u scale) differ in the last bit from fl(fl(u 0.8) / 525):
    what a kernel would write that folded the scale's division into the product.  form 0 has one operation per
    coordinate, so there is nothing a fused multiply-add could contract."""
    f = np.float32
    scale = f(f(0.8) / f(525.0))
    rng = np.random.default_rng(0xF3A)
    uv = rng.uniform(0, 640, (8192, 2)).astype(np.float32)
    exact = uv[:, 0] * scale
    folded = (uv[:, 0] * f(0.8)) / f(525.0)
    sep = np.nonzero(exact.view(np.uint32) != folded.view(np.uint32))[0]
    assert len(sep) >= 32, "no value separates u scale from (u 0.8) / 525"
    return uv[sep[:64]].copy(), scale
