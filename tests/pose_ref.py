"""POSE's LM refine arithmetic (moped_amd/csrc/pose_lm_dev.h) restated in numpy, operation for operation and in the C++
evaluation order: residual_rows / row_from_grad, lm_cost, wave_sum, the normal equations, solve6 and rotate_left.

In float32 (the default) this is what the device is held to word for word (tests/test_gpu_pose_rows.py): every operation
there is IEEE -- add, multiply, correctly rounded divide and sqrtf, no contraction.  The same code runs in float64 through
`dtype` (the twin the CPU test measures the float32 rounding against).  Two device operations have no exact numpy
counterpart: solve6's reciprocal square root (v_rsq_f32) and rotate_left's sinf / cosf.  Here they are the correctly
rounded values, and `pert` moves every one of them by that many floats (solve6: +-1, v_rsq_f32's stated accuracy;
rotate_left: the project's transcendental bound) so that a test can build its bar from the effect.

`mut` names ONE deliberate error (a one-token change) or is None; tests/test_pose_ref_cpu.py shows that its case set
notices each of them.  Points are in the kernel's layout: u, v, x, y, z [, image word | wx, wy, wz, cauchyWeight].
A camera is its DevCam: K [4], Rc [9] row major, tc [3]."""
import numpy as np

F = np.float32
FILL = 0xFFC0DE00                      # MH_POSE_DEBUG_FILL
STRIDE = {0: 5, 1: 9, 2: 9, 3: 6}      # PointStride<KIND>
PAIRS = ((0, 0), (1, 1), (2, 2), (3, 3), (1, 0), (2, 0))   # (kind, res) the refine instantiates
H_PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]  # packed index k -> (a, b)
ROW_MUTANTS = ("swap_w", "alpha", "no50", "f50_outside", "gw_cross_y", "rc_transposed", "iz_missing", "tc_kept", "cam0",
               "no2", "pen_grad")
NE_MUTANTS = ("swap_H", "hs_on_g", "hs_depth")
ORDER_MUTANTS = ("seq_wave_sum", "chunked")


def n_rows(res, phase):
    return ((2, 4, 3, 2)[res]) if phase == 0 else (3 if res == 2 else 2)


def same_words(a, b):
    """Bit for bit as uint32 words, except that a NaN equals any NaN (sign and payload are the processor's choice)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def _row_from_grad(Rc, y, gc, mut):
    """row_from_grad: gw = Rc gc, J = (y x gw, gw).  Rc [n,9], y, gc: three [n] arrays each."""
    if mut == "rc_transposed":
        gw = [gc[0] * Rc[:, k] + gc[1] * Rc[:, 3 + k] + gc[2] * Rc[:, 6 + k] for k in range(3)]
    else:
        gw = [gc[0] * Rc[:, k * 3] + gc[1] * Rc[:, k * 3 + 1] + gc[2] * Rc[:, k * 3 + 2] for k in range(3)]
    if mut == "gw_cross_y":
        rot = [gw[1] * y[2] - gw[2] * y[1], gw[2] * y[0] - gw[0] * y[2], gw[0] * y[1] - gw[1] * y[0]]
    else:
        rot = [y[1] * gw[2] - y[2] * gw[1], y[2] * gw[0] - y[0] * gw[2], y[0] * gw[1] - y[1] * gw[0]]
    return np.stack(rot + gw, axis=1)


def residual_rows(kind, res, phase, alpha, R, t, cams, pts, lst, dtype=F, mut=None, res2_penalty_row=False):
    """residual_rows<res> through cam_of<kind> for every list entry -> (nrows, r [n,4], J [n,4,6]); rows >= nrows hold 0
    here (the hook writes FILL there).  cams: (K [m,4], Rc [m,9], tc [m,3]).  res2_penalty_row: the form before the
    third row of res 2 followed the reference behind the camera (pen * w3 there, no gradient)."""
    T = dtype
    pts = np.asarray(pts, F).reshape(-1, STRIDE[kind])
    p = pts[np.asarray(lst)].astype(T)
    n = len(p)
    img = pts[np.asarray(lst), 5].view(np.int32) if (kind == 3 and mut != "cam0") else np.zeros(n, np.int64)
    K, Rc, tc = (np.asarray(a, F).astype(T)[img] for a in cams)
    R = np.asarray(R).astype(T).reshape(9)   # (float32 poses in the tests; the float64 twin also takes a perturbed float64 one)
    t = np.asarray(t).astype(T).reshape(3)
    alpha = T(F(alpha))
    one, two = T(1), T(2)
    nr = n_rows(res, phase)
    r = np.zeros((n, 4), T)
    J = np.zeros((n, 4, 6), T)
    with np.errstate(all="ignore"):
        X, Y, Z = p[:, 2], p[:, 3], p[:, 4]
        y = [R[0] * X + R[1] * Y + R[2] * Z, R[3] * X + R[4] * Y + R[5] * Z, R[6] * X + R[7] * Y + R[8] * Z]
        if mut == "tc_kept":
            wx, wy, wz = y[0] + t[0], y[1] + t[1], y[2] + t[2]
        else:
            wx, wy, wz = y[0] + t[0] - tc[:, 0], y[1] + t[1] - tc[:, 1], y[2] + t[2] - tc[:, 2]
        c = [wx * Rc[:, 0] + wy * Rc[:, 3] + wz * Rc[:, 6], wx * Rc[:, 1] + wy * Rc[:, 4] + wz * Rc[:, 7],
             wx * Rc[:, 2] + wy * Rc[:, 5] + wz * Rc[:, 8]]
        w3, w2 = np.zeros(n, T), np.ones(n, T)
        if res in (1, 2):
            w3 = (alpha if mut == "alpha" else (one - alpha)) * p[:, 8]
            w2 = one - w3
            if mut == "swap_w":
                w2, w3 = w3, w2
        behind = (c[2] < 0) | ~(np.abs(c[2]) > T(F(1e-9)))
        pen = -c[2] + T(10)
        zero = np.zeros(n, T)
        # ---- in front of the camera ----
        if res in (0, 2, 3):
            iz = one / c[2]
            du = c[0] * iz * K[:, 0] + K[:, 2] - p[:, 0]
            dv = c[1] * iz * K[:, 1] + K[:, 3] - p[:, 1]
            gu = [K[:, 0] * iz, zero, (-K[:, 0] * c[0] * iz) if mut == "iz_missing" else (-K[:, 0] * c[0] * iz * iz)]
            gv = [zero, K[:, 1] * iz, -K[:, 1] * c[1] * iz * iz]
            s0 = np.sqrt(w2) if phase == 0 else w2
            if phase == 0:
                r[:, 0], r[:, 1] = s0 * du, s0 * dv
                fu, fv = s0, s0
            else:
                r[:, 0], r[:, 1] = s0 * du * du, s0 * dv * dv
                fu, fv = (s0 * du, s0 * dv) if mut == "no2" else (two * s0 * du, two * s0 * dv)
            J[:, 0] = _row_from_grad(Rc, y, [fu * gu[k] for k in range(3)], mut)
            J[:, 1] = _row_from_grad(Rc, y, [fv * gv[k] for k in range(3)], mut)
            if res == 2:
                W = [p[:, 5], p[:, 6], p[:, 7]]
                pw = c[0] * W[0] + c[1] * W[1] + c[2] * W[2] - one
                n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
                nn = np.sqrt(n2)
                f50 = T(50)
                if phase == 0:
                    s3 = np.sqrt(w3) if mut == "no50" else (f50 * np.sqrt(w3) if mut == "f50_outside" else np.sqrt(f50 * w3))
                    r[:, 2] = s3 * nn * pw
                    g = [s3 * (c[k] / nn * pw + nn * W[k]) for k in range(3)]
                else:
                    k3 = w3 if mut == "no50" else f50 * w3
                    r[:, 2] = k3 * n2 * pw * pw
                    if mut == "no2":
                        g = [k3 * (c[k] * pw * pw + n2 * pw * W[k]) for k in range(3)]
                    else:
                        g = [k3 * (two * c[k] * pw * pw + n2 * two * pw * W[k]) for k in range(3)]
                J[:, 2] = _row_from_grad(Rc, y, g, mut)
        else:
            W = [p[:, 5], p[:, 6], p[:, 7]]
            wn = np.sqrt(W[0] * W[0] + W[1] * W[1] + W[2] * W[2])
            nv = [W[0] / wn, W[1] / wn, W[2] / wn]
            sp = nv[0] * c[0] + nv[1] * c[1] + nv[2] * c[2]
            e = [c[k] - nv[k] * sp for k in range(3)]
            ez = wn - sp
            if phase == 0:
                s2, s3 = np.sqrt(w2), np.sqrt(w3)
                for a in range(3):
                    r[:, a] = s2 * e[a]
                    J[:, a] = _row_from_grad(Rc, y, [s2 * (T(1 if a == k else 0) - nv[a] * nv[k]) for k in range(3)], mut)
                r[:, 3] = s3 * ez
                J[:, 3] = _row_from_grad(Rc, y, [-s3 * nv[k] for k in range(3)], mut)
            else:
                r[:, 0] = w2 * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
                r[:, 1] = w3 * ez * ez
                f2 = one if mut == "no2" else two
                J[:, 0] = _row_from_grad(Rc, y, [f2 * w2 * e[k] for k in range(3)], mut)
                J[:, 1] = _row_from_grad(Rc, y, [-f2 * w3 * ez * nv[k] for k in range(3)], mut)
        # ---- behind it (or within 1e-9 of its plane): the reference's penalty, no gradient ----
        pen_rows = nr if (res != 2 or res2_penalty_row) else 2   # res 2: the depth row stays what it is
        for a in range(pen_rows):
            wgt = np.ones(n, T)
            if res == 1:
                wgt = w3 if a == nr - 1 else w2
            if res == 2:
                wgt = w3 if a == 2 else w2
            r[:, a] = np.where(behind, pen * (np.sqrt(wgt) if phase == 0 else wgt), r[:, a])
            if mut == "pen_grad":
                f = np.sqrt(wgt) if phase == 0 else wgt
                Jp = _row_from_grad(Rc, y, [zero, zero, -f], None)
            else:
                Jp = np.zeros((n, 6), T)
            J[:, a] = np.where(behind[:, None], Jp, J[:, a])
    return nr, r, J


def wave_sum(v, mut=None):
    """wave_sum of a [64] vector: pairs, quads, halves of 8, rows of 16, then (r0 + r1) + (r2 + r3)."""
    v = np.asarray(v)
    assert v.shape[0] == 64
    with np.errstate(all="ignore"):
        if mut == "seq_wave_sum":
            s = v[0]
            for i in range(1, 64):
                s = s + v[i]
            return s
        for _ in range(4):
            v = v[0::2] + v[1::2]
        return (v[0] + v[1]) + (v[2] + v[3])


def _lanes(n, mut):
    """-> [steps, 64] entry numbers (-1: none): which list entry a lane takes at each step of its loop."""
    if mut == "chunked":   # lane l takes the contiguous entries [l m, (l + 1) m)
        m = -(-n // 64)
        idx = np.arange(64)[None, :] * m + np.arange(m)[:, None]
    else:                  # lane l takes l, l + 64, ...
        idx = np.arange(-(-n // 64))[:, None] * 64 + np.arange(64)[None, :]
    return np.where(idx < n, idx, -1)


def lm_cost(nr, r, mut=None):
    """lm_cost: per lane c += r[a] * r[a] over its entries in ascending order, rows in order; then the tree."""
    T = r.dtype.type
    c = np.zeros(64, T)
    with np.errstate(all="ignore"):
        for step in _lanes(len(r), mut):
            ok = step >= 0
            for a in range(nr):
                v = r[step, a]
                c = np.where(ok, c + v * v, c)
    return wave_sum(c, mut)


def normal_equations(res, phase, nr, r, J, mut=None):
    """lm_accumulate + lm_reduce -> (H [21], g [6]): per lane H[k] += J[a] J[b] (a <= b, packed row by row), g[a] += J[a] r;
    27 trees; hs = 1.5 on H for phase 1 of res 0 / 3."""
    T = r.dtype.type
    H, g = np.zeros((21, 64), T), np.zeros((6, 64), T)
    pairs = list(H_PAIRS)
    if mut == "swap_H":
        pairs[3], pairs[8] = pairs[8], pairs[3]
    with np.errstate(all="ignore"):
        for step in _lanes(len(r), mut):
            ok = step >= 0
            for row in range(nr):
                Jr, rr = J[step, row], r[step, row]
                for k, (a, b) in enumerate(pairs):
                    H[k] = np.where(ok, H[k] + Jr[:, a] * Jr[:, b], H[k])
                for a in range(6):
                    g[a] = np.where(ok, g[a] + Jr[:, a] * rr, g[a])
        hs = T(1.5) if (phase == 1 and (res in (0, 3) or mut == "hs_depth")) else T(1)
        Hs = np.array([hs * wave_sum(H[k], mut) for k in range(21)], T)
        gs = np.array([wave_sum(g[a], mut) for a in range(6)], T)
        if mut == "hs_on_g":
            gs = hs * gs
    return Hs, gs


def debug_rows(kind, res, phase, alpha, R, t, cams, pts, lst, dtype=F, mut=None, **kw):
    """Everything mh_pose_debug_rows returns, as arrays of `dtype`."""
    row_mut = mut if mut in ROW_MUTANTS else None
    sum_mut = mut if mut in NE_MUTANTS + ORDER_MUTANTS else None
    nr, r, J = residual_rows(kind, res, phase, alpha, R, t, cams, pts, lst, dtype, row_mut, **kw)
    H, g = normal_equations(res, phase, nr, r, J, sum_mut)
    return dict(nrows=nr, r=r, J=J, cost=lm_cost(nr, r, sum_mut), H=H, g=g)


def _step_floats(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def solve6(Hp, g, mu, dtype=F, pert=0, mut=None):
    """solve6 -> (ok, x [6]): Cholesky of H + mu I with the reciprocals of the diagonal, x = -(H + mu I)^-1 g.
    float32: the reciprocal square root correctly rounded, then moved by `pert` floats."""
    T = dtype
    Hp = np.asarray(Hp, F).astype(T)
    g = np.asarray(g, F).astype(T)
    A = np.zeros((6, 6), T)
    for k, (i, j) in enumerate(H_PAIRS):
        A[i, j] = A[j, i] = Hp[k]
    mu = T(F(mu))
    for i in range(6):
        A[i, i] = A[i, i] + mu
    L, inv = np.zeros((6, 6), T), np.zeros(6, T)
    x = np.zeros(6, T)
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i + 1):
                s = A[i, j]
                for m in range(j):
                    if mut == "drop_term" and (i, j, m) == (4, 3, 1):
                        continue
                    s = s - L[i, m] * L[j, m]
                if i == j:
                    if not s > 0:
                        return False, x
                    if T is F:
                        inv[i] = _step_floats(F(1.0 / np.sqrt(np.float64(s))), pert)
                    else:
                        inv[i] = T(1) / np.sqrt(s)
                    L[i, i] = s * inv[i]
                else:
                    L[i, j] = s * inv[j]
        y = np.zeros(6, T)
        for i in range(6):
            s = g[i] if mut == "plus_g" else -g[i]
            for m in range(i):
                s = s - L[i, m] * y[m]
            y[i] = s * inv[i]
        for i in range(5, -1, -1):
            s = y[i]
            for m in range(i + 1, 6):
                s = s - L[m, i] * x[m]
            x[i] = s * inv[i]
    return True, x


def rotate_left(w, R, dtype=F, pert=0, mut=None):
    """rotate_left -> exp([w]x) R as [9].  float32: sinf / cosf correctly rounded, then moved by `pert` floats."""
    T = dtype
    w = np.asarray(w, F).astype(T)[:3]
    R = np.asarray(R, F).astype(T).reshape(9)
    with np.errstate(all="ignore"):
        th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        th = np.sqrt(th2)
        if th < T(F(1e-4)):
            a = T(1) - th2 / T(6)
            b = T(0.5) - th2 / T(24)
        else:
            if T is F:
                s, c = _step_floats(F(np.sin(np.float64(th))), pert), _step_floats(F(np.cos(np.float64(th))), -pert)
            else:
                s, c = np.sin(th), np.cos(th)
            a = s / th
            b = (T(1) - c) / (th if mut == "b_th" else th2)
        z = T(0)
        K = [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]
        if mut == "transpose_K":
            K = [K[0], K[3], K[6], K[1], K[4], K[7], K[2], K[5], K[8]]
        K2 = [K[r * 3] * K[c_] + K[r * 3 + 1] * K[3 + c_] + K[r * 3 + 2] * K[6 + c_] for r in range(3) for c_ in range(3)]
        E = [a * K[i] + b * K2[i] for i in range(9)]
        for i in (0, 4, 8):
            E[i] = E[i] + T(1)
        out = [E[r * 3] * R[c_] + E[r * 3 + 1] * R[3 + c_] + E[r * 3 + 2] * R[6 + c_] for r in range(3) for c_ in range(3)]
    return np.array(out, T)


def debug_step(H, g, mu, R, t, dtype=F, pert_rsq=0, pert_trig=0, mut=None):
    """mh_pose_debug_step -> (ok, dx [6], Rn [9], tn [3]); solve6's mutants / rotate_left's by name."""
    ok, dx = solve6(H, g, mu, dtype, pert_rsq, mut if mut in ("drop_term", "plus_g") else None)
    if not ok:
        return False, None, None, None
    Rn = rotate_left(dx, R, dtype, pert_trig, mut if mut in ("b_th", "transpose_K") else None)
    tn = np.asarray(t, F).astype(dtype) + dx[3:]
    return True, dx, Rn, tn


def step_f64(H, g, mu, R, t):
    """The float64 reference of a step on the float32 inputs: numpy.linalg.solve, Rodrigues' formula -> (dx, Rn [9], tn)."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(H_PAIRS):
        A[i, j] = A[j, i] = np.float64(F(H[k]))
    A = A + np.float64(F(mu)) * np.eye(6)
    dx = np.linalg.solve(A, -np.asarray(g, F).astype(np.float64))
    return dx, rodrigues(dx[:3]) @ np.asarray(R, F).astype(np.float64).reshape(3, 3), np.asarray(t, F).astype(np.float64) + dx[3:]


def rodrigues(w):
    """exp([w]x) in float64."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + Kx + 0.5 * Kx @ Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
