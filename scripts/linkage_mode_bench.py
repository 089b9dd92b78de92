#!/usr/bin/env python3
"""mh_cluster_linkage in its two modes (mh_linkage_set_mode: SCAN, one workgroup per problem that rescans every live pair
per merge, against ROWMAX, the matrix stage on the whole grid and the merge loop over cached row maxima), one problem
per call, the "scene" points of tests/test_gpu_linkage_stages.py over its depth map, moped3d's parameters (cutoff 0.1,
MinPts 7, Use3DFilter 2, average linkage, automatic sigmas):

  * n = 150, 586 (the size of the bundled frame's planar list), 1024 in both modes, alternating, five rounds;
  * n = 2048 and 4096 in ROWMAX alone (SCAN refuses them);
  * per case the matrix stage and the agglomeration separately: the call with a cutoff no similarity reaches (the matrix
    stage, the first scan, the upload of the points and the labels back) and the call with the real cutoff; the
    difference is the merge loop.  Device events on the context's stream around each call, the median of `reps` calls
    per round;
  * merges and rescanned rows per merge of the ROWMAX call, from mh_linkage_stats.

    python scripts/linkage_mode_bench.py [out.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from moped_amd import capi  # noqa: E402
import test_gpu_linkage_stages as stages  # noqa: E402

MODES = (("SCAN", capi.LINKAGE_SCAN), ("ROWMAX", capi.LINKAGE_ROWMAX))
ROUNDS = 5


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    maps = stages.make_maps()
    img, fill = (torch.from_numpy(a).to(dev) for a in maps["scene"])
    c = capi.Context(0)
    st = torch.cuda.Stream()                 # (not torch's default stream: its handle is 0, which mh_set_stream reads as "your own")
    c.set_stream(st.cuda_stream)
    torch.cuda.set_stream(st)
    c.frame_set_depth_image(img.data_ptr(), fill.data_ptr(), stages.W, stages.H, capi.DEPTH_BACKPROJECTION, 0.5, 0.1)

    def ms(fn, reps):
        fn()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    lines = ["mh_cluster_linkage, one problem per call, ms (device events; median of the calls of a round; %d rounds, the modes "
             "alternating): matrix = the call with cutoff +inf, merge loop = the call with cutoff 0.1 minus that" % ROUNDS]
    for n in (150, 586, 1024, 2048, 4096):
        _, uv, mx, world = stages.family_case("scene", n, maps)
        modes = MODES if n <= 1024 else MODES[1:]
        reps = 20 if n <= 1024 else 5
        full, none = capi.default_linkage_params(), capi.default_linkage_params()
        none.cutoff = float("inf")
        res = {name: ([], []) for name, _ in modes}
        for _ in range(ROUNDS):
            for name, mode in modes:
                c.linkage_set_mode(mode)
                t_matrix = ms(lambda: c.cluster_linkage([(uv, mx, world)], none), reps)
                t_full = ms(lambda: c.cluster_linkage([(uv, mx, world)], full), reps)
                res[name][0].append(t_matrix)
                res[name][1].append(t_full - t_matrix)
        c.linkage_set_mode(capi.LINKAGE_ROWMAX)
        c.linkage_stats(reset=True)
        (clusters, _), = c.cluster_linkage([(uv, mx, world)], full)
        _, merges, rescans, _ = c.linkage_stats()
        c.linkage_set_mode(capi.LINKAGE_SCAN)
        for name, _ in modes:
            lines.append("n = %4d  %-6s  matrix %s   merge loop %s" % (n, name, " / ".join("%.3f" % v for v in res[name][0]),
                                                                       " / ".join("%.3f" % v for v in res[name][1])))
            print(lines[-1], flush=True)
        lines.append("n = %4d  ROWMAX: %d merges, %.2f rows rescanned per merge, %d clusters" % (n, merges, rescans / max(merges, 1), len(clusters)))
        print(lines[-1], flush=True)
    c.frame_set_depth_image(0, 0, 0, 0, 0)
    c.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
