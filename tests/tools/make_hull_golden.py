"""Makes tests/golden/hull_ref.npz: clouds of 2-D points and what the reference's own getConvexHull
(moped2/libmoped/include/moped.hpp:293-327) returns for them.

    python tests/tools/make_hull_golden.py [<reference tree>]        (default: $MOPED_REFERENCE or /root/reference)

Builds tests/tools/hull_golden_harness.cpp against the reference header where it lies, in a temporary directory, runs
it on the clouds below and packs inputs and recorded outputs.  Needed only to remake the golden; no test runs it.

Families (the `family` array indexes FAMILIES):
  small      1 .. 7 random points (one point -> the empty hull; two -> both)
  empty      no point at all: undefined in the reference (*points.begin()), recorded as the empty hull the device gives
  equal      2 .. 40 copies of one point
  collinear  points on a horizontal, a vertical or a diagonal line of integers, with repeats
  lattice    300 clouds on small integer lattices: every determinant exact, ties everywhere
  uniform    300 uniform clouds of 8 .. 64 points in a 640 x 480 image
  projected  24 box clouds of 100 .. 5 000 model points projected (the oracle's project()) at poses 0.5 .. 1.5 m away
  circle     points on a circle (every one a vertex), alone and with a cloud inside
The file stays near 300 KB: the projected clouds are its bulk."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
FAMILIES = ["small", "empty", "equal", "collinear", "lattice", "uniform", "projected", "circle"]
K = np.array([525.0, 525.0, 320.0, 240.0], np.float32)
CAM = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


def random_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.5)])
    return np.concatenate([q, t]).astype(np.float32)


def clouds():
    import orclib
    rng = np.random.default_rng(0x4011)
    out = []

    def add(family, pts):
        out.append((FAMILIES.index(family), np.ascontiguousarray(pts, np.float32).reshape(-1, 2)))

    for n in range(1, 8):
        for _ in range(6):
            add("small", rng.uniform(0, 100, (n, 2)))
        add("small", rng.integers(0, 3, (n, 2)))
    add("empty", np.zeros((0, 2)))
    for n in (2, 3, 4, 7, 40):
        add("equal", np.tile(rng.uniform(-50, 50, (1, 2)), (n, 1)))
    add("equal", np.tile([[0.0, -0.0]], (5, 1)))
    for n in (2, 3, 5, 17, 64):
        t = rng.integers(-20, 20, n).astype(np.float32)
        add("collinear", np.stack([t, np.full(n, 7.0)], 1))
        add("collinear", np.stack([np.full(n, -3.0), t], 1))
        add("collinear", np.stack([t, 2 * t + 1], 1))
        add("collinear", np.stack([t, -t], 1))
    for _ in range(300):
        side = int(rng.integers(2, 13))
        add("lattice", rng.integers(0, side, (int(rng.integers(3, 81)), 2)) - side // 2)
    for _ in range(300):
        add("uniform", rng.uniform(0, 1, (int(rng.integers(8, 65)), 2)) * [640, 480])
    sizes = [100, 5000] + [int(np.exp(rng.uniform(np.log(100), np.log(5000)))) for _ in range(22)]
    for n in sizes:
        dims = rng.uniform(0.05, 0.3, 3)
        xyz = (rng.uniform(-0.5, 0.5, (n, 3)) * dims).astype(np.float32)
        add("projected", orclib.project(random_pose(rng), xyz, K, CAM))
    for n in (3, 8, 64, 200, 777):
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        ring = np.stack([320 + 200 * np.cos(a), 240 + 200 * np.sin(a)], 1)
        add("circle", rng.permutation(ring))
        add("circle", rng.permutation(np.concatenate([ring, [320, 240] + rng.uniform(-100, 100, (n, 2))])))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOPED_REFERENCE", "/root/reference")
    inc = os.path.join(ref, "moped2", "libmoped", "include")
    cs = clouds()
    off = np.concatenate([[0], np.cumsum([len(p) for _, p in cs])]).astype(np.int32)
    pts = np.concatenate([p for _, p in cs]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("harness", "in.bin", "out.bin"))
        subprocess.check_call(["g++", "-O2", "-w", "-std=gnu++98", "-fno-delete-null-pointer-checks", "-I", inc,
                               os.path.join(HERE, "hull_golden_harness.cpp"), "-o", exe])
        with open(fin, "wb") as f:
            f.write(np.int32(len(cs)).tobytes() + off.tobytes() + pts.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = np.fromfile(fout, np.int32)
    n = int(raw[0])
    assert n == len(cs)
    hoff = raw[1:n + 2].copy()
    hull = raw[n + 2:].view(np.float32).reshape(-1, 2).copy()
    assert len(hull) == hoff[-1]
    path = os.path.join(ROOT, "tests", "golden", "hull_ref.npz")
    np.savez_compressed(path, families=np.array(FAMILIES), family=np.array([f for f, _ in cs], np.int8), off=off,
                        pts=pts, hoff=hoff, hull=hull)
    print(f"{path}: {n} clouds, {len(pts)} points, {len(hull)} hull vertices, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
