"""python scripts/wms_kernel_bench.py [CALLS]

Times mh_cluster_wms at n = 150, 586, 2048 (MaxIterations 100): host clock around the synchronous call (upload, launch,
download, ends in a stream synchronise), two runs per size.  Under rocprofv3 --kernel-trace the same script
gives the kernel's own time: dispatches come in blocks of WARM + 2 * CALLS + 1 (the debug-state call) per size, in SIZES order."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from moped_amd import capi  # noqa: E402
from make_wms_golden import scene, fills  # noqa: E402

SIZES = (150, 586, 2048)
WARM = 3
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def main():
    rng = np.random.default_rng(11)
    ctx = capi.Context(0)
    prm = capi.mh_wms_params(0.1, 0.02, 7, 100, 10.0)
    probs = {n: [(scene(rng, n, 4 if n > 200 else 2), fills(rng, n))] for n in SIZES}
    runs = {n: [[], []] for n in SIZES}
    for n in SIZES:
        for _ in range(WARM):
            ctx.cluster_wms(probs[n], prm)
        for r in range(2):
            for _ in range(CALLS):
                t0 = time.perf_counter()
                cl = ctx.cluster_wms(probs[n], prm)
                runs[n][r].append(time.perf_counter() - t0)
        st = ctx.wms_debug_state(probs[n], prm)[0]
        print(f"n={n}: clusters {len(cl[0])}, members {sum(len(m) for m in cl[0])}, active {int(st[2].sum())}, iterations {st[3]}")
    for n in SIZES:
        a, b = (np.median(r) * 1e3 for r in runs[n])
        print(f"n={n}: call time median run A {a:.3f} ms, run B {b:.3f} ms (min {min(map(min, runs[n])) * 1e3:.3f} ms), {CALLS} calls each")
    ctx.close()


if __name__ == "__main__":
    main()
