"""Reference of the scale fit (include/scale/hc_pose_scale.h), in numpy only.

The rule of the header's comment restated from its text, steps 1 to 4, in
np.float32: numpy rounds every operation and never contracts, so the integers
(voter, counts, mask bits) and the scale's bits are the ones the rule defines.
fit64 is the same method in float64, for the CPU tests that bound what the
float32 rounding may change.  The joint mask of step 1 is refine_reference's
float32 restatement of the 2 px test.
"""
import numpy as np

import refine_reference as RR

NONE, NO_VOTER = 1, 2
MARGIN = 0.01   # px: an edgel this close to the 2 px gate may fall on either side in another precision
POSE_KEYS = RR.POSE_KEYS


def _pose(pose, dtype):
    if isinstance(pose, dict):
        pose = tuple(pose[k] for k in POSE_KEYS)
    return tuple(np.asarray(x, dtype).reshape(-1) for x in pose)


def _edgels(loc, K, pose, f):
    """Step 2 for all E edgels in the float type f (no masks applied):
    rho, Y (3 arrays), s, and the view-3 observation in pixels."""
    R21, t21, R31, t31 = pose
    loc = np.asarray(loc, f)
    K = np.asarray(K, f).reshape(9)
    g0, g1, h0, h1, q0, q1 = (loc[:, i] for i in range(6))
    one, zero = f(1), f(0)
    with np.errstate(all="ignore"):
        a = ((zero + R21[2] * h0) + R21[5] * h1) + R21[8] * one
        rho = t21[2] * a
        rho = rho - (((zero + R21[2] * t21[0]) + R21[5] * t21[1]) + R21[8] * t21[2])
        m2 = ((zero + R21[6] * g0) + R21[7] * g1) + R21[8] * one
        rho = rho / (one - m2 * a)
        X = (rho * g0, rho * g1, rho)
        Y = tuple(((zero + R31[3 * i] * X[0]) + R31[3 * i + 1] * X[1]) + R31[3 * i + 2] * X[2] for i in range(3))
        a0, a1, a2 = q1 * Y[2] - one * Y[1], one * Y[0] - q0 * Y[2], q0 * Y[1] - q1 * Y[0]
        b0, b1, b2 = q1 * t31[2] - one * t31[1], one * t31[0] - q0 * t31[2], q0 * t31[1] - q1 * t31[0]
        s = -(((a0 * b0 + a1 * b1) + a2 * b2) / ((b0 * b0 + b1 * b1) + b2 * b2))
        p0, p1 = q0 * K[0] + K[2], q1 * K[4] + K[5]
    assert s.dtype == f and Y[0].dtype == f
    return rho, Y, s, (p0, p1)


def _error(Y, p, s, t31, K, f):
    """Step 3 without its gate: (Z2, the pixel error) of the given edgels under scale s."""
    K = np.asarray(K, f).reshape(9)
    with np.errstate(all="ignore"):
        Z0, Z1, Z2 = Y[0] + s * t31[0], Y[1] + s * t31[1], Y[2] + s * t31[2]
        d0 = ((Z0 / Z2) * K[0] + K[2]) - p[0]
        d1 = ((Z1 / Z2) * K[4] + K[5]) - p[1]
        err = np.sqrt((d0 * d0 + d1 * d1) + f(0) * f(0))
    return Z2, err


def _fit(pose, loc, K, f, scale_in, has_path=True):
    pose32 = _pose(pose, np.float32)
    E = len(loc)
    out = dict(status=0, num_voters=0, voter=-1, transfer_inliers=0, tested=0, joint=0,
               scale_in=np.float32(scale_in), scale31=np.float32(scale_in), key=0, mask=np.zeros(E, bool),
               counts=np.zeros(0, np.int64), voters=np.zeros(0, np.int64))
    if not has_path:
        out["status"] = NONE
        return out
    m21, m31 = RR.score(loc, K, pose32)                       # step 1: always the float32 test
    m = m21 & m31
    P = _pose(pose, f)
    rho, Y, s, p = _edgels(loc, K, P, f)
    tested = m & (rho > 0)
    voters = np.nonzero(tested & np.isfinite(s) & (s > 0))[0]
    out.update(joint=int(m.sum()), tested=int(tested.sum()), num_voters=len(voters), voters=voters)
    if len(voters) == 0:
        out["status"] = NO_VOTER
        return out
    idx = np.nonzero(tested)[0]
    Yt, pt = tuple(y[idx] for y in Y), tuple(x[idx] for x in p)
    counts = np.zeros(len(voters), np.int64)
    near = np.zeros(len(voters), np.int64)                    # per voter: tested edgels within MARGIN px of the gate
    for j, v in enumerate(voters):                            # vectorised per voter
        Z2, err = _error(Yt, pt, s[v], P[3], K, f)
        counts[j] = int(((Z2 > 0) & (err < f(2))).sum())
        near[j] = int((np.abs(err - f(2)) <= f(MARGIN)).sum())
    out["near"] = near
    keys = (counts << 32) | voters
    w = int(np.argmax(keys))
    v = int(voters[w])
    Z2, err = _error(Yt, pt, s[v], P[3], K, f)
    mask = np.zeros(E, bool)
    mask[idx[(Z2 > 0) & (err < f(2))]] = True
    out.update(voter=v, transfer_inliers=int(counts[w]), scale31=s[v], key=int(keys[w]), mask=mask, counts=counts,
               err=err, tested_idx=idx)
    assert int(mask.sum()) == int(counts[w])
    return out


def fit(pose, loc, K, scale_in=0.0, has_path=True):
    """The rule in float32.  pose: dict or tuple (R21, t21, R31, t31).  Returns
    a dict with the hcScaleReport's fields, mask ((E,) bool), voters and counts
    (c_v per voter)."""
    r = _fit(pose, np.ascontiguousarray(loc, np.float32), K, np.float32, scale_in, has_path)
    assert r["scale31"].dtype == np.float32
    return r


def fit64(pose, loc, K, scale_in=0.0):
    """The same method with steps 2 to 4 in float64 (the joint mask stays the
    float32 test's): what the rule would give without rounding."""
    return _fit(pose, np.ascontiguousarray(loc, np.float32), K, np.float64, scale_in)


def pack(mask):
    """(E,) bool -> the (E + 63) // 64 uint64 words of a device mask."""
    E = len(mask)
    bits = np.zeros(((E + 63) // 64) * 64, np.uint8)
    bits[:E] = mask
    return np.packbits(bits, bitorder="little").view(np.uint64)
