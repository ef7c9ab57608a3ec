"""Reference of the three-view refinement (include/threeview/hc_pose_threeview.h),
in numpy only.

The rule of the header restated: Gauss-Newton on eleven local parameters (view
2's five, view 3's five, the log of the scale) over the fit set F, with the
view-2 pixel residual and the three-view transfer residual stacked, F and every
count recomputed at every iterate, the iterate with the most transfer inliers
returned.

The counting is np.float32 through refine_reference.score (the 2 px test) and
scale_reference._edgels / _error (steps 2 and 3 of the scale header); everything
else is float64.  The Jacobian is by central differences through the update
itself with step 1e-6, so it shares no derivative code with the kernel, which
differentiates analytically.
"""
import numpy as np

import refine_reference as RR
import scale_reference as SR

MAX_ITERATIONS = RR.MAX_ITERATIONS
NONE, TOO_FEW, SINGULAR, SKIPPED = 1, 2, 4, 8
DAMPING = RR.DAMPING
FD_STEP = RR.FD_STEP
MARGIN = SR.MARGIN
POSE_KEYS = RR.POSE_KEYS
NPAR = 11


def transfer_residuals(g, h, q, state, s, K):
    """The pixel error of Z = R31 (rho (g0, g1, 1)) + s t31 against the view-3
    observation q, rho the view-1-2 depth, all in double: (E, 2)."""
    (R21, t21), (R31, t31) = state
    K0, K2, K4, K5 = (float(K[i]) for i in (0, 2, 4, 5))
    c = R21[:, 2]
    a = c[0] * h[:, 0] + c[1] * h[:, 1] + c[2]
    m2 = R21[2, 0] * g[:, 0] + R21[2, 1] * g[:, 1] + R21[2, 2]
    rho = (t21[2] * a - c @ t21) / (1.0 - m2 * a)
    M = g[:, 0:1] * R31[:, 0] + g[:, 1:2] * R31[:, 1] + R31[:, 2]          # (E, 3) = R31 gamma1
    Z = M * rho[:, None] + s * t31
    return np.stack([(Z[:, 0] / Z[:, 2] * K0 + K2) - (q[:, 0] * K0 + K2),
                     (Z[:, 1] / Z[:, 2] * K4 + K5) - (q[:, 1] * K4 + K5)], axis=1)


def apply(state, s, d):
    """The update: d = (w2, u2, w3, u3, sigma)."""
    return [RR.apply(state[0][0], state[0][1], d[0:5]), RR.apply(state[1][0], state[1][1], d[5:10])], \
        s * float(np.exp(d[10]))


def _rows(l64, state, s, K):
    """The four residual rows per edgel, flattened edgel by edgel: (4 E,)."""
    g, h, q = l64[:, 0:2], l64[:, 2:4], l64[:, 4:6]
    r2 = RR.residuals(g, h, state[0][0], state[0][1], K)
    rT = transfer_residuals(g, h, q, state, s, K)
    return np.concatenate([r2, rT], axis=1)


def normal_equations(l64, state, s, K):
    """(A, grad, sse of the view-2 rows, sse of the transfer rows) over the given edgels."""
    r = _rows(l64, state, s, K)
    J = np.zeros((r.shape[0], 4, NPAR))
    for p in range(NPAR):
        d = np.zeros(NPAR)
        d[p] = FD_STEP
        sp, cp = apply(state, s, d)
        sm, cm = apply(state, s, -d)
        J[:, :, p] = (_rows(l64, sp, cp, K) - _rows(l64, sm, cm, K)) / (2.0 * FD_STEP)
    J = J.reshape(-1, NPAR)
    return J.T @ J, J.T @ r.reshape(-1), float((r[:, 0:2] ** 2).sum()), float((r[:, 2:4] ** 2).sum())


def solve(A, grad):
    """(A + 1e-9 diag A) d = -grad by Cholesky, refine_reference.solve at any
    size; None when a pivot is not positive or a value is not finite."""
    n = len(grad)
    M = A + DAMPING * np.diag(np.diag(A))
    if not (np.isfinite(M).all() and np.isfinite(grad).all()):
        return None
    L = np.zeros((n, n))
    for j in range(n):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0.0:
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (-grad[i] - L[i, :i] @ y[:i]) / L[i, i]
    d = np.zeros(n)
    for i in range(n - 1, -1, -1):
        d[i] = (y[i] - L[i + 1:, i] @ d[i + 1:]) / L[i, i]
    return d if np.isfinite(d).all() else None


def count(loc, K, p32, s32):
    """Step 1 of an iterate, in float32: the masks (m21, m31, F, T) of the pose
    floats p32 and the float scale s32."""
    f = np.float32
    m21, m31 = RR.score(loc, K, p32)
    rho, Y, _, p = SR._edgels(loc, K, p32, f)
    tested = m21 & m31 & (rho > 0)
    Z2, err = SR._error(Y, p, f(s32), p32[3], K, f)
    F = tested & (Z2 > 0)
    return m21, m31, F, F & (err < f(2))


def near_gate(loc, K, state, s):
    """Edgels whose float64 error lies within MARGIN of the 2 px gate in view 2,
    in view 3 or in the transfer: the ones a state that differs in its last bits
    may count otherwise."""
    l64 = np.asarray(loc, np.float64)
    g = l64[:, 0:2]
    with np.errstate(all="ignore"):
        rs = [RR.residuals(g, l64[:, 2:4], state[0][0], state[0][1], K),
              RR.residuals(g, l64[:, 4:6], state[1][0], state[1][1], K),
              transfer_residuals(g, l64[:, 2:4], l64[:, 4:6], state, s, K)]
        n = np.zeros(len(l64), bool)
        for r in rs:
            n |= np.abs(np.hypot(r[:, 0], r[:, 1]) - 2.0) <= MARGIN
    return int(n.sum())


def refine3(sel, loc, K, iterations=10, min_inliers=16):
    """sel: a dict with R21, t21, R31, t31 (float32), scale31 and the counts
    inliers, inliers21, inliers31 of a selection that stages 1 and 2 produced
    (a path and a fitted scale).  Returns a dict: the best iterate's pose floats,
    scale31 (float32), inliers, inliers21, inliers31 (the input's own when the
    best iterate is 0), fit_set, transfer_inliers, status, iterations_run,
    best_iteration, transfer_history and joint_history (33,), near (33,: the
    edgels near a gate at that iterate), scale_in, rms_px_in and rms_px_out
    (2,: view-2 rows, transfer rows), state64 and scale64 of the best iterate,
    and iterates, per scored iterate its floats, counts, rms and transfer mask."""
    loc = np.ascontiguousarray(loc, np.float32)
    K = np.asarray(K, np.float32).reshape(9)
    l64 = loc.astype(np.float64)
    state = [(np.asarray(sel["R21"], np.float64).reshape(3, 3), np.asarray(sel["t21"], np.float64)),
             (np.asarray(sel["R31"], np.float64).reshape(3, 3), np.asarray(sel["t31"], np.float64))]
    s = float(np.float32(sel["scale31"]))
    histT = np.full(MAX_ITERATIONS + 1, -1, np.int32)
    histJ = np.full(MAX_ITERATIONS + 1, -1, np.int32)
    near = np.zeros(MAX_ITERATIONS + 1, np.int64)
    status, best, rms_in, k, iterates = 0, None, np.zeros(2), 0, []
    while True:
        p32 = tuple(x.astype(np.float32).reshape(-1) for Rt in state for x in Rt)
        s32 = np.float32(s)
        m21, m31, F, T = count(loc, K, p32, s32)
        cT, nF = int(T.sum()), int(F.sum())
        histT[k], histJ[k] = cT, int((m21 & m31).sum())
        near[k] = near_gate(loc, K, state, s)
        A, grad, sse2, sseT = normal_equations(l64[F], state, s, K)
        rms = np.sqrt(np.array([sse2, sseT]) / nF) if nF > 0 else np.zeros(2)
        if k == 0:
            rms_in = rms
        iterates.append(dict(R21=p32[0], t21=p32[1], R31=p32[2], t31=p32[3], scale31=s32, inliers=int(histJ[k]),
                             inliers21=int(m21.sum()), inliers31=int(m31.sum()), fit_set=nF, transfer_inliers=cT,
                             rms_px=rms, mask=T))
        if best is None or cT >= best["transfer_inliers"]:
            best = dict(R21=p32[0], t21=p32[1], R31=p32[2], t31=p32[3], scale31=s32, inliers=int(histJ[k]),
                        inliers21=int(m21.sum()), inliers31=int(m31.sum()), fit_set=nF, transfer_inliers=cT,
                        best_iteration=k, rms_px_out=rms, state64=[(R.copy(), t.copy()) for R, t in state],
                        scale64=s, mask=T)
        if nF < min_inliers:
            status |= TOO_FEW
            break
        if k == iterations:
            break
        d = solve(A, grad)
        if d is None:
            status |= SINGULAR
            break
        state, s = apply(state, s, d)
        k += 1
    if best["best_iteration"] == 0:                       # the stage-2 values, bit for bit
        best.update({c: int(sel[c]) for c in ("inliers", "inliers21", "inliers31") if c in sel})
    best.update(status=status, iterations_run=k, transfer_history=histT, joint_history=histJ, near=near,
                scale_in=np.float32(sel["scale31"]), rms_px_in=rms_in, iterates=iterates)
    return best
