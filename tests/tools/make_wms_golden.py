"""Makes tests/golden/wms_ref.npz: point sets with fill distances and what the reference's own
CLUSTER_WEIGHTED_MEAN_SHIFT_CPU (moped3d/libmoped/src/cluster/CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp) makes of them.

    python tests/tools/make_wms_golden.py [<reference tree>]        (default: $MOPED_REFERENCE or /root/reference)

Builds tests/tools/wms_golden_harness.cpp twice against the reference headers where they lie, in a temporary directory:
plain (process() as a pipeline calls it -> the clusters) and instrumented (the same, and per image the weights, the final
centres, the active flags and the iteration count, observed without touching the header; see the harness).  Both builds
must give the same clusters.  Needed only to remake the golden; no test runs it.

Coordinates are multiples of 1/4096 and fill distances small integers or halves so that the file stays small (~250 KB).

Families (the `family` array indexes FAMILIES); a case is ONE model's match list, images = its FrameData::images.size():
  sizes      n = 0, 1, MinPts, MinPts + 1 (a tight blob: the strict `>` decides), 63 / 64 / 65, 1023 / 1024 / 1025, 2048
  blobs      2 .. 5 blobs with 20 % outliers, several (Radius, Merge)
  dup        every point four times
  lattice    points on a lattice of spacing 1/8 with Radius and Merge exactly 1/8 or one ulp above: the strict `<` decides
  radius0    Radius = 0: every centre 0/0 after one iteration, nothing is emitted
  iter       MaxIterations = 0 (one cluster per point around the raw points) and 1
  fill       fill distances all 0, all -1, large against a small halfWeightDistance, halfWeightDistance = 0
  nan        NaN coordinates in some points
  images     two or three images, imageIdx interleaved (one image empty)
  overlap    large Radius, small Merge: points in several clusters (members / points up to ~2.7)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FAMILIES = ["sizes", "blobs", "dup", "lattice", "radius0", "iter", "fill", "nan", "images", "overlap"]


def quant(a):
    return (np.round(np.asarray(a, np.float64) * 4096) / 4096).astype(np.float32)


def scene(rng, n, blobs=3, sigma=0.03, outliers=0.2):
    """n points: `blobs` Gaussian blobs in front of a camera, a share of uniform outliers, in random order."""
    n_out = int(round(n * outliers))
    ctr = np.stack([rng.uniform(-0.5, 0.5, blobs), rng.uniform(-0.4, 0.4, blobs), rng.uniform(0.6, 1.4, blobs)], 1)
    which = rng.integers(0, blobs, n - n_out)
    pts = ctr[which] + rng.normal(0, sigma, (n - n_out, 3))
    out = np.stack([rng.uniform(-0.7, 0.7, n_out), rng.uniform(-0.6, 0.6, n_out), rng.uniform(0.4, 1.6, n_out)], 1)
    return quant(rng.permutation(np.concatenate([pts, out])))


def fills(rng, n):
    """a Kinect frame's mix: most matches on measured pixels (0), some filled from 0.5 .. 30 px away, a few unknown (-1)"""
    f = np.zeros(n, np.float32)
    k = rng.random(n)
    far = k > 0.6
    f[far] = rng.integers(1, 61, int(far.sum())) / 2
    f[k > 0.95] = -1
    return f


def cases():
    rng = np.random.default_rng(0x3D5)
    out = []

    def add(family, xyz, fill=None, R=0.1, M=0.02, hwd=10.0, min_pts=7, max_iter=100, image=None, images=1):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        fill = fills(rng, n) if fill is None else np.ascontiguousarray(np.broadcast_to(np.asarray(fill, np.float32), (n,)))
        image = np.zeros(n, np.int32) if image is None else np.asarray(image, np.int32)
        out.append(dict(family=FAMILIES.index(family), prm=np.array([R, M, hwd], np.float32),
                        iprm=np.array([min_pts, max_iter, images], np.int32), xyz=xyz, fill=fill, image=image))

    add("sizes", np.zeros((0, 3)))
    add("sizes", scene(rng, 1, 1, 0.01, 0))
    add("sizes", scene(rng, 7, 1, 0.005, 0))    # MinPts points in one canopy: size 7 is not > 7
    add("sizes", scene(rng, 8, 1, 0.005, 0))    # MinPts + 1: kept
    for n in (63, 64, 65):
        add("sizes", scene(rng, n, 2))
    for n in (1023, 1024, 1025, 2048):
        add("sizes", scene(rng, n, 4))
    for R, M in ((0.1, 0.02), (0.15, 0.05), (0.2, 0.03)):
        for n, b in ((150, 2), (586, 5)):
            add("blobs", scene(rng, n, b), R=R, M=M)
    add("dup", np.repeat(scene(rng, 40, 2), 4, axis=0))
    add("dup", rng.permutation(np.repeat(scene(rng, 30, 2), 4, axis=0)))
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(2), indexing="ij"), -1).reshape(-1, 3) / 8.0 + [0, 0, 1]
    up = float(np.nextafter(np.float32(0.125), np.float32(1)))
    for R, M in ((0.125, 0.125), (up, 0.125), (0.125, up), (up, up)):
        add("lattice", g, fill=0, R=R, M=M, min_pts=0, max_iter=20)
    add("lattice", rng.permutation(g), fill=0, R=up, M=up, min_pts=2, max_iter=20)
    add("radius0", scene(rng, 50, 2), R=0.0, max_iter=5)
    add("radius0", scene(rng, 50, 2), R=0.0, max_iter=5, min_pts=0)
    s = scene(rng, 150, 3)
    add("iter", s, max_iter=0)
    add("iter", s, max_iter=1)
    add("iter", s, max_iter=2)
    s = scene(rng, 200, 3)
    add("fill", s, fill=0)
    add("fill", s, fill=-1)
    add("fill", s, fill=rng.integers(1000, 1000000, 200), hwd=0.5)
    add("fill", s, hwd=0.5)
    add("fill", s, hwd=0.0)                     # (d * d) / 0: weights 0 (or NaN where d is 0 too)
    add("fill", s, fill=rng.integers(1, 50, 200), hwd=0.0)   # every weight 0: every centre 0/0
    s = scene(rng, 100, 2).copy()
    s[[3, 40, 41, 77, 99], [0, 1, 2, 0, 1]] = np.nan
    add("nan", s)
    s[0] = np.nan
    add("nan", s, min_pts=0)
    s = scene(rng, 200, 3)
    add("images", s, image=np.arange(200) % 2, images=2)
    add("images", s, image=rng.integers(0, 2, 200) * 2, images=3)   # image 1 has no match
    add("images", scene(rng, 21, 1, 0.01, 0), image=[0] * 9 + [1] * 12, images=2)
    s = scene(rng, 300, 3, 0.05)
    add("overlap", s, R=0.3, M=0.005)
    add("overlap", s, R=0.3, M=0.01)
    add("overlap", s, R=0.5, M=0.01)
    add("overlap", scene(rng, 64, 2, 0.1), R=1.0, M=0.001)
    return out


def run(exe, cs, tmp, instrumented):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    off = np.concatenate([[0], np.cumsum([len(c["xyz"]) for c in cs])]).astype(np.int32)
    with open(fin, "wb") as f:
        f.write(np.int32(len(cs)).tobytes())
        f.write(np.stack([c["prm"] for c in cs]).tobytes())
        f.write(np.stack([c["iprm"] for c in cs]).tobytes())
        f.write(off.tobytes())
        for key in ("xyz", "fill", "image"):
            f.write(np.concatenate([c[key] for c in cs]).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, np.int32)
    n = int(raw[0])
    assert n == len(cs)
    pos = 1
    ncl = raw[pos:pos + n].copy()
    pos += n
    n_all = int(raw[pos])
    pos += 1
    cl_off = raw[pos:pos + n_all + 1].copy()
    pos += n_all + 1
    members = raw[pos:pos + cl_off[-1]].copy()
    pos += int(cl_off[-1])
    res = dict(off=off, ncl=ncl, cl_off=cl_off, members=members)
    if instrumented:
        n_prob = int(raw[pos])
        pos += 1
        poff = raw[pos:pos + n_prob + 1].copy()
        pos += n_prob + 1
        tot = int(poff[-1])
        res["poff"] = poff
        res["iterations"] = raw[pos:pos + n_prob].copy()
        pos += n_prob
        res["weight"] = raw[pos:pos + tot].view(np.float32).copy()
        pos += tot
        res["centre"] = raw[pos:pos + 3 * tot].view(np.float32).reshape(-1, 3).copy()
        pos += 3 * tot
        res["active"] = raw[pos:pos + tot].astype(np.int8)
        pos += tot
    assert pos == len(raw)
    return res


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOPED_REFERENCE", "/root/reference")
    lib = os.path.join(ref, "moped3d", "libmoped")
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        res = []
        for instrumented in (False, True):
            exe = os.path.join(tmp, "harness%d" % instrumented)
            subprocess.check_call(["g++", "-O2", "-w", "-std=gnu++98", "-fno-delete-null-pointer-checks",
                                   "-I", os.path.join(lib, "include"), "-I", os.path.join(lib, "src", "cluster")]
                                  + (["-DWMS_INSTRUMENT"] if instrumented else [])
                                  + [os.path.join(HERE, "wms_golden_harness.cpp"), "-o", exe])
            res.append(run(exe, cs, tmp, instrumented))
    plain, ins = res
    for key in ("ncl", "cl_off", "members"):
        assert np.array_equal(plain[key], ins[key]), f"the two builds disagree on {key}"
    assert len(ins["iterations"]) == sum(int(c["iprm"][2]) for c in cs)
    path = os.path.join(ROOT, "tests", "golden", "wms_ref.npz")
    np.savez_compressed(path, families=np.array(FAMILIES), family=np.array([c["family"] for c in cs], np.int8),
                        prm=np.stack([c["prm"] for c in cs]), iprm=np.stack([c["iprm"] for c in cs]),
                        xyz=np.concatenate([c["xyz"] for c in cs]), fill=np.concatenate([c["fill"] for c in cs]),
                        image=np.concatenate([c["image"] for c in cs]).astype(np.int8), **ins)
    pts = int(ins["off"][-1])
    print(f"{path}: {len(cs)} cases, {pts} points, {len(ins['cl_off']) - 1} clusters, {len(ins['members'])} members "
          f"({len(ins['members']) / max(pts, 1):.2f} per point), {os.path.getsize(path)} bytes")
    for f, name in enumerate(FAMILIES):
        idx = [i for i, c in enumerate(cs) if c["family"] == f]
        k0 = np.concatenate([[0], np.cumsum(ins["ncl"])])
        mem = sum(int(ins["cl_off"][k0[i + 1]] - ins["cl_off"][k0[i]]) for i in idx)
        print(f"  {name:8s} {len(idx):2d} cases, {sum(len(cs[i]['xyz']) for i in idx):5d} points, "
              f"{sum(int(ins['ncl'][i]) for i in idx):4d} clusters, {mem:6d} members")


if __name__ == "__main__":
    main()
