"""The case set of POSE's refine arithmetic, shared by tests/test_pose_ref_cpu.py (restatement <-> oracle <-> float64) and
tests/test_gpu_pose_rows.py (device <-> restatement, bit for bit).  Deterministic; nothing here calls the code under test.

A case is one scene -- a pose, three cameras, points with their pixels, depth-map attributes and image numbers, a list
of point indices, alpha -- from which points(case, kind) lays out the kernel's point array for a kind.  Kinds 0..2 see
cams[0] only; kind 3 sees all three, the points interleaved over them.

family "front":  every point at depth >= 0.3 m (in float64) in its camera.
family "behind": every third point 0.3 .. 1.5 m BEHIND its camera, the rest in front.
family "edge":   identity pose and camera, so that the camera-frame point IS the model point, exactly: depths -0., 0.,
                 5e-10, the float above 1e-9, one ordinary point, and one with a zero depth-map vector W (kind 1: NaN rows;
                 the reference divides by |W| as well).  Compared with hand-worked rows on the CPU, bit for bit on the GPU.
"""
import numpy as np

F = np.float32
LENGTHS = (1, 3, 63, 64, 65, 128, 129, 320, 2048)
ALPHAS = (0.0, 0.5, 1.0)
CAUCHY = (0.0, 0.3, 1.0)


def quat(axis, angle):
    """-> float32 (x, y, z, w), normalised in float64 and rounded."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    q = np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])
    return q.astype(F)


def tm_init(q):
    """TransformMatrix::init in float32, operation for operation (geom.h tm_from_pose, oracle.cpp tm_init) -> R [9]."""
    q0, q1, q2, q3 = (F(v) for v in q)
    two, one = F(2), F(1)
    return np.array([one - two * q1 * q1 - two * q2 * q2, two * q0 * q1 - two * q3 * q2, two * q0 * q2 + two * q3 * q1,
                     two * q0 * q1 + two * q3 * q2, one - two * q0 * q0 - two * q2 * q2, two * q1 * q2 - two * q3 * q0,
                     two * q0 * q2 - two * q3 * q1, two * q1 * q2 + two * q3 * q0, one - two * q0 * q0 - two * q1 * q1], F)


def devcams(cams):
    """make_devcam for [(K, cam7), ...] -> (K [m,4], Rc [m,9], tc [m,3]) float32."""
    K = np.array([c[0] for c in cams], F).reshape(-1, 4)
    Rc = np.array([tm_init(c[1][:4]) for c in cams], F)
    tc = np.array([c[1][4:] for c in cams], F).reshape(-1, 3)
    return K, Rc, tc


CAM_I = (np.array([520.0, 515.0, 320.5, 240.25], F), np.array([0, 0, 0, 1, 0, 0, 0], F))
CAM_A = (np.array([610.0, 598.5, 301.75, 255.5], F), np.concatenate([quat([0.3, -1.0, 0.2], 0.6), F([0.10, -0.05, 0.20])]).astype(F))
CAM_B = (np.array([480.25, 470.0, 350.0, 200.5], F), np.concatenate([quat([1.0, 0.4, -0.3], -0.45), F([-0.25, 0.10, 0.05])]).astype(F))
CAM_C = (np.array([700.0, 705.5, 330.25, 260.0], F), np.concatenate([quat([-0.2, 0.5, 1.0], 0.8), F([0.05, 0.20, -0.15])]).astype(F))


def _scene(name, family, n_pts, lst, seed, cam0, alpha, px, pose=True):
    rng = np.random.default_rng(seed)
    cams = [cam0, CAM_B, CAM_C]
    K, Rc, tc = (a.astype(np.float64) for a in devcams(cams))
    q = quat([0.5, 0.2, -1.0], 0.7) if pose else F([0, 0, 0, 1])
    t = F([0.08, -0.12, 0.9]) if pose else F([0, 0, 0])
    R = tm_init(q).astype(np.float64).reshape(3, 3)
    img = (np.arange(n_pts) % 3).astype(np.int32)
    # camera-frame points inside a frustum, then back into model coordinates: once through cams[0] for every point (what
    # kinds 0..2 see) and once through cams[img] (kind 3), so that each kind finds its pixels where its camera projects
    z = rng.uniform(0.3, 1.5, n_pts)
    if family == "behind":
        z[::3] = -z[::3]
    c = np.stack([rng.uniform(-0.35, 0.35, n_pts) * np.abs(z), rng.uniform(-0.3, 0.3, n_pts) * np.abs(z), z], axis=1)
    noise = rng.normal(0.0, px, (n_pts, 2))

    def place(cam_of):
        xyz, uv = np.empty((n_pts, 3)), np.empty((n_pts, 2))
        for i, m in enumerate(cam_of):
            xyz[i] = R.T @ (Rc[m].reshape(3, 3) @ c[i] + tc[m] - t.astype(np.float64))
            uv[i] = [c[i, 0] / c[i, 2] * K[m, 0] + K[m, 2], c[i, 1] / c[i, 2] * K[m, 1] + K[m, 3]]
        return xyz.astype(F), (uv + noise).astype(F)

    xyz, uv = place(np.zeros(n_pts, np.int32))
    xyz3, uv3 = place(img)
    # depth-map attributes (kinds 1, 2: cams[0]).  kind 1: W = the camera-frame point as the depth map saw it (1 % off along
    # the ray, 3 mm across); kind 2: W with p . W = 1 up to the same 1 % (the class's depth row is |p| |p . W - 1|).  The
    # depth map's point lies in front of the camera also where the pose puts the model point behind it.
    off = 1.0 + rng.normal(0.0, 0.01, n_pts)
    cf = c * np.sign(c[:, 2:3])
    W1 = (cf * off[:, None] + rng.normal(0.0, 0.003, (n_pts, 3))).astype(F)
    W2 = (cf / np.sum(cf * cf, axis=1, keepdims=True) * off[:, None]).astype(F)
    wgt = np.array(CAUCHY, F)[(np.arange(n_pts) // 2) % 3]
    return dict(name=name, family=family, q=q, t=t, R=tm_init(q), cams=cams, uv=uv, xyz=xyz, uv3=uv3, xyz3=xyz3, W1=W1, W2=W2, wgt=wgt, img=img,
                lst=np.asarray(lst, np.int32), alpha=float(alpha), px=px)


def _edge():
    s = _scene("edge", "edge", 6, np.arange(6), 77, CAM_I, 0.5, 0.3, pose=False)
    z = np.array([-0.0, 0.0, 5e-10, np.nextafter(F(1e-9), F(1)), 0.8, 0.9], F)
    s["xyz"] = np.stack([F([0.05, -0.02, 0.03, 0.01, 0.10, -0.07]), F([0.01, 0.04, -0.06, 0.02, -0.05, 0.08]), z], axis=1).astype(F)
    s["uv"] = F([[330, 250], [300, 200], [310, 260], [340, 230], [385.75, 207.5], [280.0, 286.25]])
    s["xyz3"], s["uv3"] = s["xyz"], s["uv"]
    s["img"] = np.zeros(6, np.int32)            # (identity camera for kind 3 as well)
    s["W1"] = F([[0.1, 0.1, 1], [0.1, 0, 1], [0, 0.1, 1], [0.05, 0.05, 1], [0.1, -0.05, 0.81], [0, 0, 0]])
    s["W2"] = F([[0.1, 0.1, 1], [0.1, 0, 1], [0, 0.1, 1], [0.05, 0.05, 1], [0.15, -0.08, 1.22], [0, 0, 0]])
    s["wgt"] = F([0.3, 1.0, 0.3, 1.0, 0.3, 1.0])
    return s


def _build():
    out = []
    for i, n in enumerate(LENGTHS):   # every length once, the other attributes cycling through their values
        out.append(_scene(f"n{n}", "front", n, np.arange(n), 100 + i, CAM_I if i % 2 else CAM_A, ALPHAS[i % 3], (0.3, 50.0)[(i // 2) % 2]))
    out.append(_scene("permuted129", "front", 129, np.random.default_rng(5).permutation(129), 201, CAM_A, 0.5, 50.0))
    out.append(_scene("sparse65", "front", 200, 3 * np.arange(65) + 2, 202, CAM_I, 0.0, 50.0))
    rep = np.arange(65)
    rep[6] = rep[5]
    rep[64] = rep[0]
    out.append(_scene("repeated65", "front", 65, rep, 203, CAM_A, 1.0, 0.3))
    for i, alpha in enumerate(ALPHAS):
        out.append(_scene(f"behind{i}", "behind", 70, np.arange(70), 300 + i, CAM_A if i != 1 else CAM_I, alpha, 50.0))
    out.append(_edge())
    return out


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}


def points(case, kind):
    """The kernel's point array for `kind`: float32 words [n_pts, stride]."""
    n = len(case["xyz"])
    cols = [case["uv3"], case["xyz3"]] if kind == 3 else [case["uv"], case["xyz"]]
    if kind == 3:
        cols.append(case["img"].astype(np.int32).view(F).reshape(n, 1))
    elif kind in (1, 2):
        cols += [case["W1"] if kind == 1 else case["W2"], case["wgt"].reshape(n, 1)]
    return np.ascontiguousarray(np.concatenate([np.asarray(c, F).reshape(n, -1) for c in cols], axis=1), F)


def depth64(case, kind):
    """Depth of every LIST ENTRY in the camera its kind projects it through, in float64 from the float32 inputs."""
    K, Rc, tc = (a.astype(np.float64) for a in devcams(case["cams"]))
    R = case["R"].astype(np.float64).reshape(3, 3)
    out = np.empty(len(case["lst"]))
    for j, i in enumerate(case["lst"]):
        m = case["img"][i] if kind == 3 else 0
        w = R @ case["xyz3" if kind == 3 else "xyz"][i].astype(np.float64) + case["t"].astype(np.float64) - tc[m]
        out[j] = Rc[m].reshape(3, 3)[:, 2] @ w
    return out


def pose7(case):
    return np.concatenate([case["q"], case["t"]]).astype(F)
