"""Which small kernel holds the compute units that passes A / B cannot use?  Reads the workgroup records scripts/cu_trace.py
saved (CU_TRACE_SAVE=file.npy: {kernel, compute unit, t0, t1} of every workgroup; needs no GPU) and prints, next to that
script's three shares of CU time, per small kernel:
  union   -- CU time during which at least one of the kernel's workgroups is resident on the CU (a union per CU: the
             "CU-ms" column of cu_trace.py is the sum of the workgroups' durations and counts a CU with three of them thrice),
  alone   -- CU time during which the kernel's workgroups are the ONLY ones resident on the CU (nothing of passes A / B,
             nothing of another small kernel): what this kernel by itself keeps from the passes,
  no pass -- CU time during which the kernel is resident and no pass A / B workgroup is (other small kernels may be).
usage: cu_trace_attrib.py records.npy [records2.npy ...]"""
import sys

import numpy as np

NAMES = {1: "normalize", 2: "prepare", 3: "pass A", 4: "tau", 5: "pass B", 6: "pass C", 7: "group", 8: "CLUSTER", 9: "POSE", 10: "other"}
BIG = (3, 5)
NK = 11


def attribute(r):
    r = r[(r[:, 0] >> np.uint64(32)) <= np.uint64(10)]
    kid = (r[:, 0] >> np.uint64(32)).astype(np.int64)
    hw = (r[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    xcc = (r[:, 1] & np.uint64(0xF)).astype(np.int64)
    ta, tb = r[:, 2].astype(np.int64), r[:, 3].astype(np.int64)
    cu = (xcc << 8) | ((hw >> 8) & 0xFF)
    lo, hi = int(np.quantile(ta, 0.2)), int(np.quantile(tb, 0.8))   # the steady window of cu_trace.py
    cus = np.unique(cu)
    union = np.zeros(NK)
    alone = np.zeros(NK)
    nopass = np.zeros(NK)
    t_big = t_small = t_any = 0
    for c in cus:
        m = cu == c
        a, b, k = np.clip(ta[m], lo, hi), np.clip(tb[m], lo, hi), kid[m]
        keep = b > a
        a, b, k = a[keep], b[keep], k[keep]
        # events sorted by time, ends before starts at the same tick
        t = np.concatenate([a, b])
        d = np.concatenate([np.ones(len(a), np.int64), -np.ones(len(b), np.int64)])
        kk = np.concatenate([k, k])
        order = np.lexsort((d, t))
        t, d, kk = t[order], d[order], kk[order]
        cnt = np.zeros(NK, np.int64)
        last = lo
        for ti, di, ki in zip(t.tolist(), d.tolist(), kk.tolist()):
            dt = ti - last
            if dt > 0:
                n_big = cnt[3] + cnt[5]
                n_all = int(cnt.sum())
                if n_big > 0:
                    t_big += dt
                elif n_all > 0:
                    t_small += dt
                if n_all > 0:
                    t_any += dt
                res = np.nonzero(cnt)[0]
                union[res] += dt
                if n_big == 0:
                    nopass[res] += dt
                if len(res) == 1:
                    alone[res[0]] += dt
                last = ti
            cnt[ki] += di
    denom = len(cus) * (hi - lo)
    inwin = (tb > lo) & (ta < hi)
    print(f"window {(hi - lo) * 1e-5:.2f} ms, {len(cus)} compute units, {int(inwin.sum())} workgroups")
    print(f"CU time: {100 * t_big / denom:.1f}% with a pass A/B workgroup resident, {100 * t_small / denom:.1f}% with only "
          f"small-kernel workgroups, {100 * (1 - t_any / denom):.1f}% empty")
    print(f"{'kernel':10s} {'workgroups':>10s} {'sum CU-ms':>10s} {'union CU-ms':>12s} {'share':>7s} {'no pass CU-ms':>14s} {'share':>7s} "
          f"{'alone CU-ms':>12s} {'share':>7s}")
    for kx in sorted(NAMES):
        mk = inwin & (kid == kx)
        if not mk.any():
            continue
        s = (np.minimum(tb[mk], hi) - np.maximum(ta[mk], lo)).sum() * 1e-5
        print(f"{NAMES[kx]:10s} {int(mk.sum()):10d} {s:10.2f} {union[kx] * 1e-5:12.2f} {100 * union[kx] / denom:6.2f}% "
              f"{nopass[kx] * 1e-5:14.2f} {100 * nopass[kx] / denom:6.2f}% {alone[kx] * 1e-5:12.2f} {100 * alone[kx] / denom:6.2f}%")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for path in sys.argv[1:]:
        print(f"== {path}")
        attribute(np.load(path))
