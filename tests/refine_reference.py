"""Reference of the pose refinement (hc_trifocal_pose_refine), in numpy only.

The method of include/refine/hc_pose_refine.h restated: Gauss-Newton on the
pixel reprojection residuals of the edgels that are joint inliers, the inlier
set recomputed at every iterate, the best-scoring iterate returned.

Scoring runs in np.float32, op for op as reproj_inlier of
csrc/hc_pose_device.hpp (numpy rounds every operation and never contracts);
everything else in float64.  The Jacobian is by central differences through the
update itself (R <- Exp(w) R, t <- normalize(t + u0 b1 + u1 b2)), so it shares
no derivative code with the kernel, which differentiates analytically.
"""
import numpy as np

MAX_ITERATIONS = 32
NONE, TOO_FEW, SINGULAR = 1, 2, 4
DAMPING = 1e-9
FD_STEP = 1e-6
POSE_KEYS = ("R21", "t21", "R31", "t31")


# ---- scoring: float32, the ops of reproj_inlier in their order ---------------

def inliers_f32(g, h, R, T, K):
    """g, h (E, 2) float32; R (9,), T (3,), K (9,) float32 -> (E,) bool."""
    f = np.float32
    g0, g1, h0, h1 = g[:, 0], g[:, 1], h[:, 0], h[:, 1]
    R = np.asarray(R, f)
    T = np.asarray(T, f)
    K0, K2, K4, K5 = (f(K[i]) for i in (0, 2, 4, 5))
    with np.errstate(all="ignore"):
        a = ((f(0) + R[2] * h0) + R[5] * h1) + R[8] * f(1)
        rho = T[2] * a
        b = ((f(0) + R[2] * T[0]) + R[5] * T[1]) + R[8] * T[2]
        rho = rho - b
        m0 = ((f(0) + R[0] * g0) + R[1] * g1) + R[2] * f(1)
        m1 = ((f(0) + R[3] * g0) + R[4] * g1) + R[5] * f(1)
        m2 = ((f(0) + R[6] * g0) + R[7] * g1) + R[8] * f(1)
        rho = rho / (f(1) - m2 * a)
        m0 = m0 * rho + T[0]
        m1 = m1 * rho + T[1]
        m2 = m2 * rho + T[2]
        m0 = m0 / m2
        m1 = m1 / m2
        m0 = m0 * K0 + K2
        m1 = m1 * K4 + K5
        m0 = m0 - (h0 * K0 + K2)
        m1 = m1 - (h1 * K4 + K5)
        err = np.sqrt((m0 * m0 + m1 * m1) + f(0) * f(0))
    assert err.dtype == np.float32
    return err < f(2)


def score(loc, K, pose32):
    """pose32 = (R21, t21, R31, t31) float32 -> (m21, m31) bool masks."""
    loc = np.asarray(loc, np.float32)
    return (inliers_f32(loc[:, 0:2], loc[:, 2:4], pose32[0], pose32[1], K),
            inliers_f32(loc[:, 0:2], loc[:, 4:6], pose32[2], pose32[3], K))


# ---- the residual and the local parameters: float64 --------------------------

def residuals(g, h, R, t, K):
    """The pixel residual m - p of reproj_inlier in double: (E, 2)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64)
    K0, K2, K4, K5 = (float(K[i]) for i in (0, 2, 4, 5))
    c = R[:, 2]
    a = c[0] * h[:, 0] + c[1] * h[:, 1] + c[2]
    rho = t[2] * a - c @ t
    m = g[:, 0:1] * R[:, 0] + g[:, 1:2] * R[:, 1] + R[:, 2]          # (E, 3) = R gamma1
    rho = rho / (1.0 - m[:, 2] * a)
    q = m * rho[:, None] + t
    return np.stack([(q[:, 0] / q[:, 2] * K0 + K2) - (h[:, 0] * K0 + K2),
                     (q[:, 1] / q[:, 2] * K4 + K5) - (h[:, 1] * K4 + K5)], axis=1)


def exp_so3(w):
    th = float(np.linalg.norm(w))
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * (W @ W)
    return np.eye(3) + (np.sin(th) / th) * W + ((1.0 - np.cos(th)) / (th * th)) * (W @ W)


def tangent_basis(t):
    i = int(np.argmin(np.abs(t)))          # the first of equal minima
    e = np.zeros(3)
    e[i] = 1.0
    b1 = np.cross(t, e)
    b1 = b1 / np.linalg.norm(b1)
    return b1, np.cross(t, b1)


def apply(R, t, d):
    """The update of one view: d = (w0, w1, w2, u0, u1)."""
    b1, b2 = tangent_basis(t)
    tn = t + d[3] * b1 + d[4] * b2
    return exp_so3(d[:3]) @ R, tn / np.linalg.norm(tn)


def normal_equations(g, h, R, t, K):
    """(A, grad, sse) of one view over the given edgels, J by central differences."""
    r = residuals(g, h, R, t, K)
    J = np.zeros((r.shape[0], 2, 5))
    for p in range(5):
        d = np.zeros(5)
        d[p] = FD_STEP
        Rp, tp = apply(R, t, d)
        Rm, tm = apply(R, t, -d)
        J[:, :, p] = (residuals(g, h, Rp, tp, K) - residuals(g, h, Rm, tm, K)) / (2.0 * FD_STEP)
    J = J.reshape(-1, 5)
    r = r.reshape(-1)
    return J.T @ J, J.T @ r, float(r @ r)


def solve(A, grad):
    """(A + 1e-9 diag A) d = -grad by Cholesky; None when a pivot is not
    positive or a value is not finite."""
    M = A + DAMPING * np.diag(np.diag(A))
    if not (np.isfinite(M).all() and np.isfinite(grad).all()):
        return None
    L = np.zeros((5, 5))
    for j in range(5):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0.0:
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 5):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(5)
    for i in range(5):
        y[i] = (-grad[i] - L[i, :i] @ y[:i]) / L[i, i]
    d = np.zeros(5)
    for i in range(4, -1, -1):
        d[i] = (y[i] - L[i + 1:, i] @ d[i + 1:]) / L[i, i]
    return d if np.isfinite(d).all() else None


def refine(pose32, loc, K, iterations=10, min_inliers=16):
    """pose32: dict or tuple with R21 (9,), t21 (3,), R31 (9,), t31 (3,) float32
    (a selection with a path).  Returns a dict: the best iterate's R21, t21, R31,
    t31 (the float32 values that were scored), inliers, inliers21, inliers31,
    status, iterations_run, best_iteration, joint_history (33,), rms_px_in,
    rms_px_out (2,), and pose64, the best iterate's float64 state."""
    if isinstance(pose32, dict):
        pose32 = tuple(pose32[k] for k in ("R21", "t21", "R31", "t31"))
    loc = np.ascontiguousarray(loc, np.float32)
    K = np.asarray(K, np.float32).reshape(9)
    l64 = loc.astype(np.float64)
    g, hs = l64[:, 0:2], (l64[:, 2:4], l64[:, 4:6])
    state = [(np.asarray(pose32[2 * v], np.float64).reshape(3, 3), np.asarray(pose32[2 * v + 1], np.float64))
             for v in range(2)]
    hist = np.full(MAX_ITERATIONS + 1, -1, np.int32)
    status, best, rms_in, k = 0, None, np.zeros(2), 0
    while True:
        p32 = tuple(x.astype(np.float32).reshape(-1) for Rt in state for x in Rt)
        m21, m31 = score(loc, K, p32)
        mJ = m21 & m31
        cJ = int(mJ.sum())
        hist[k] = cJ
        systems = [normal_equations(g[mJ], hs[v][mJ], state[v][0], state[v][1], K) for v in range(2)]
        rms = np.array([np.sqrt(s[2] / cJ) if cJ > 0 else 0.0 for s in systems])
        if k == 0:
            rms_in = rms
        if best is None or cJ >= best["inliers"]:
            best = dict(R21=p32[0], t21=p32[1], R31=p32[2], t31=p32[3], inliers=cJ, inliers21=int(m21.sum()),
                        inliers31=int(m31.sum()), best_iteration=k, rms_px_out=rms,
                        pose64=[(R.copy(), t.copy()) for R, t in state], mask=mJ)
        if cJ < min_inliers:
            status |= TOO_FEW
            break
        if k == iterations:
            break
        ds = [solve(s[0], s[1]) for s in systems]
        if ds[0] is None or ds[1] is None:
            status |= SINGULAR
            break
        state = [apply(state[v][0], state[v][1], ds[v]) for v in range(2)]
        k += 1
    best.update(status=status, iterations_run=k, joint_history=hist, rms_px_in=rms_in)
    return best


def pose_distance(a, b):
    """max over the views of |R_a - R_b|_F and |t_a - t_b|_2, in float64."""
    d = 0.0
    for k in ("R21", "t21", "R31", "t31"):
        d = max(d, float(np.linalg.norm(np.asarray(a[k], np.float64).ravel() - np.asarray(b[k], np.float64).ravel())))
    return d


def borderline(loc, K, pose64, margin=0.01, gate=2.0):
    """Edgels whose float64 error under pose64 lies within margin of the gate in
    either view: the ones another summation order may flip."""
    l64 = np.asarray(loc, np.float64)
    n = np.zeros(l64.shape[0], bool)
    for v in range(2):
        r = residuals(l64[:, 0:2], l64[:, 2 + 2 * v:4 + 2 * v], pose64[v][0], pose64[v][1], K)
        n |= np.abs(np.hypot(r[:, 0], r[:, 1]) - gate) <= margin
    return int(n.sum())


# ---- test poses ---------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def gt_pose(data):
    """The ground-truth pose of a RansacData as the floats of a selection (unit t)."""
    return {"R21": np.asarray(data.pose21[:9], np.float32), "t21": _unit(data.pose21[9:]).astype(np.float32),
            "R31": np.asarray(data.pose31[:9], np.float32), "t31": _unit(data.pose31[9:]).astype(np.float32)}


def perturbed(pose, angle=3e-4):
    """Both rotations turned and both translation directions tilted by angle."""
    p = {}
    for v, axis in (("21", 0), ("31", 1)):
        w = np.zeros(3)
        w[axis] = angle
        R = exp_so3(w) @ np.asarray(pose["R" + v], np.float64).reshape(3, 3)
        t = np.asarray(pose["t" + v], np.float64)
        b1, _ = tangent_basis(t)
        p["R" + v] = R.reshape(-1).astype(np.float32)
        p["t" + v] = _unit(t + np.tan(angle) * b1).astype(np.float32)
    return p
