"""Reference of the structure stage (include/structure/hc_pose_structure.h), in
numpy only.

The rule of the header's comment restated from its text, steps 1 to 6, in
np.float32: numpy rounds every operation and never contracts, so the set W, the
flags and every float of a record are the ones the rule defines.  Steps 1 to 3
of the scale header (the joint mask, rho, Y, the transfer error) are
scale_reference's.  reconstruct64 is the same method in float64 on float64
inputs (W stays the float32 rule's), for the CPU tests that bound what the
float32 rounding does.
"""
import numpy as np

import refine_reference as RR
import scale_reference as SR

TANGENT, ORIENTED = 1, 2
NONE = 1
POSE_KEYS = RR.POSE_KEYS
DTYPE = np.dtype([("X", "<f4", (3,)), ("T", "<f4", (3,)), ("err3_px", "<f4"), ("sin_plane", "<f4"), ("sin3", "<f4"),
                  ("edgel", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert DTYPE.itemsize == 48


def transfer_set(pose, scale31, loc, K):
    """Step 1 in float32: (E,) bool, the edgels of W."""
    pose32 = SR._pose(pose, np.float32)
    loc = np.ascontiguousarray(loc, np.float32)
    m21, m31 = RR.score(loc, K, pose32)
    rho, Y, _, p = SR._edgels(loc, K, pose32, np.float32)
    Z2, err = SR._error(Y, p, np.float32(scale31), pose32[3], K, np.float32)
    with np.errstate(invalid="ignore"):
        return (m21 & m31) & (rho > 0) & (Z2 > 0) & (err < np.float32(2))


def _all_edgels(pose, scale31, loc, tan, K, f, min_sin_plane, max_sin3):
    """Steps 2 to 5 for all E edgels in the float type f: a dict of arrays."""
    R21, t21, R31, t31 = SR._pose(pose, f)
    loc, tan = np.asarray(loc, f), np.asarray(tan, f)
    Kf = np.asarray(K, f).reshape(9)
    s = f(scale31)
    zero = f(0)
    g0, g1, h0, h1 = (loc[:, i] for i in range(4))
    a0, a1, b0, b1, c0, c1 = (tan[:, i] for i in range(6))
    with np.errstate(all="ignore"):
        rho, Y, _, p = SR._edgels(loc, K, (R21, t21, R31, t31), f)
        X = (rho * g0, rho * g1, rho)
        Z = tuple(Y[i] + s * t31[i] for i in range(3))
        _, err = SR._error(Y, p, s, t31, K, f)
        n1 = [-a1, a0, g0 * a1 - g1 * a0]
        m = (-b1, b0, h0 * b1 - h1 * b0)
        n2 = [((zero + R21[i] * m[0]) + R21[3 + i] * m[1]) + R21[6 + i] * m[2] for i in range(3)]
        l1 = np.sqrt((n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2])
        l2 = np.sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2])
        n1 = [x / l1 for x in n1]
        n2 = [x / l2 for x in n2]
        D = (n1[1] * n2[2] - n1[2] * n2[1], n1[2] * n2[0] - n1[0] * n2[2], n1[0] * n2[1] - n1[1] * n2[0])
        sp = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
        defined = np.isfinite(sp) & (sp >= f(min_sin_plane))
        T = [d / sp for d in D]
        flip = (T[0] - T[2] * g0) * a0 + (T[1] - T[2] * g1) * a1 < zero
        T = [np.where(flip, -t, t) for t in T]
        V = [((zero + R31[3 * i] * T[0]) + R31[3 * i + 1] * T[1]) + R31[3 * i + 2] * T[2] for i in range(3)]
        p0, p1 = (V[0] * Z[2] - Z[0] * V[2]) * Kf[0], (V[1] * Z[2] - Z[1] * V[2]) * Kf[4]
        o0, o1 = c0 * Kf[0], c1 * Kf[4]
        sin3 = np.abs(p0 * o1 - p1 * o0) / (np.sqrt(p0 * p0 + p1 * p1) * np.sqrt(o0 * o0 + o1 * o1))
        sin3 = np.where(defined, sin3, f(1))
        T = [np.where(defined, t, zero) for t in T]
        oriented = defined & (sin3 < f(max_sin3))
    for x in (*X, *T, err, sp, sin3):
        assert x.dtype == f
    return dict(X=np.stack(X, 1), T=np.stack(T, 1), err3_px=err, sin_plane=sp, sin3=sin3,
                flags=defined * TANGENT + oriented * ORIENTED)


def _pick(all_e, W, scale31, dtype):
    idx = np.nonzero(W)[0]
    rec = np.zeros(len(idx), dtype)
    for k in ("X", "T", "err3_px", "sin_plane", "sin3", "flags"):
        rec[k] = all_e[k][idx]
    rec["edgel"] = idx
    rep = dict(status=0, count=len(idx), tangents=int(((rec["flags"] & TANGENT) != 0).sum()),
               oriented=int(((rec["flags"] & ORIENTED) != 0).sum()), scale31=np.float32(scale31))
    return rec, rep


def reconstruct(pose, scale31, loc, tan, K, min_sin_plane=0.05, max_sin3=0.05, has_path=True, fitted=True):
    """The rule in float32.  pose: dict or tuple (R21, t21, R31, t31); fitted:
    False when stage 2 reported HC_SCALE_NONE or HC_SCALE_NO_VOTER.  Returns
    (records, a DTYPE array in edgel order; the report as a dict)."""
    if not (has_path and fitted):
        return np.zeros(0, DTYPE), dict(status=NONE, count=0, tangents=0, oriented=0, scale31=np.float32(scale31))
    loc = np.ascontiguousarray(loc, np.float32)
    tan = np.ascontiguousarray(tan, np.float32)
    s = np.float32(scale31)
    W = transfer_set(pose, s, loc, K)
    return _pick(_all_edgels(pose, s, loc, tan, K, np.float32, min_sin_plane, max_sin3), W, s, DTYPE)


DTYPE64 = np.dtype([("X", "<f8", (3,)), ("T", "<f8", (3,)), ("err3_px", "<f8"), ("sin_plane", "<f8"), ("sin3", "<f8"),
                    ("edgel", "<i4"), ("flags", "<i4"), ("pad", "<i4")])


def reconstruct64(pose, scale31, loc, tan, K, min_sin_plane=0.05, max_sin3=0.05):
    """The same method with steps 2 to 5 in float64 on the float64 inputs given;
    W is the float32 rule's on the inputs rounded to float32."""
    W = transfer_set(pose, np.float32(scale31), loc, K)
    all_e = _all_edgels(pose, scale31, loc, tan, K, np.float64, min_sin_plane, max_sin3)
    return _pick(all_e, W, scale31, DTYPE64)
