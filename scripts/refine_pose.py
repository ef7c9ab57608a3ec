#!/usr/bin/env python3
"""The joint selection as selected against the same selection refined on its
joint inliers, on the config-5 protocol (development tool, GPU).  Prints one
JSON line.

Protocol of bench.py's noisy_pose leg: dataset 000 with sigma = 1 px noise,
trial t uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each
of 100, 300 and 1000 samples.  In every run the device tracks are scored by
hc_trifocal_pose_support_joint and its selection goes through
hc_trifocal_pose_refine (10 iterations, min_inliers 16); the verdict of each is
hc_pose_residuals against the ground truth.  Reported per size: successes and
rate with the Wilson 95 % interval before and after, the runs whose verdict
changed in each direction, the per-trial verdicts, the median rotation
residuals and joint inlier counts before and after, the refinements' status
and best iteration, and the time of the refine call beside the joint pose
call on the last run: HIP events, the two calls interleaved within a
repetition, REPS repetitions after one warm-up; median, min and max in ms.

    python scripts/refine_pose.py [TRIALS [REPS]]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import wilson95  # noqa: E402
from trifocal_pose_estimation_using_improved_gpuhc_amd import (_abi, load_problem, load_ransac_data, pose,  # noqa: E402
                                                               prepare_target_params, synthcurves)
from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker  # noqa: E402

SIZES = (100, 300, 1000)
SIGMA = 1.0
trials = int(sys.argv[1]) if len(sys.argv) > 1 else 30
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
dev = torch.device("cuda:0")
problem = load_problem()
data = load_ransac_data(0)
tr = DeviceTracker(problem, dev)
noisy = [synthcurves.noisy(data, SIGMA, synthcurves.DEFAULT_SEED + t) for t in range(trials)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def rate(ok):
    k = int(np.sum(ok))
    return {"successes": k, "success_rate": round(k / len(ok), 4), "success_rate_95ci": wilson95(k, len(ok))}


def med(rows, col):
    return round(float(np.median([r[col] for r in rows])), 5)


out = {"build_id": _abi.build_id(), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
       "workload": "config 5 protocol: Triplet_Edgels_000, sigma = %g px (noise seed 20250215 + trial), samples "
                   "srand(trial); the joint selection and the same selection refined (10 iterations, "
                   "min_inliers 16)" % SIGMA,
       "trials": trials, "reps": reps, "sizes": []}
for total in SIZES:
    res = tr.allocate(total, stats=False)
    n = total * 312
    inl3 = torch.empty((n, 3), dtype=torch.int32, device=dev)
    sel3 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    ref3 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    ok_j, ok_r, res_j, res_r, cnt_j, cnt_r, status, best_it = [], [], [], [], [], [], [], []
    for t in range(trials):
        nd = noisy[t]
        ta, da, _ = prepare_target_params(problem, nd, seed=t, num_samples=total)
        tr.set_ransac_data(nd)
        tr.reset_tracks(res)
        tr.launch(torch.from_numpy(ta).to(dev), torch.from_numpy(da).to(dev), res, num_samples=total)
        pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3)
        _, report = pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref3)
        torch.cuda.synchronize(dev)
        j = pose.joint_selection_dict(pose.joint_selection_struct(sel3))
        r = pose.joint_selection_dict(pose.joint_selection_struct(ref3))
        rep = pose.refine_report_dict(report)
        assert r["inliers"] >= j["inliers"] and r["path"] == j["path"]
        rj, okj = pose.residuals(nd, j)
        rr, okr = pose.residuals(nd, r)
        ok_j.append(bool(okj))
        ok_r.append(bool(okr))
        res_j.append([float(v) for v in rj])
        res_r.append([float(v) for v in rr])
        cnt_j.append(int(j["inliers"]))
        cnt_r.append(int(r["inliers"]))
        status.append(int(rep["status"]))
        best_it.append(int(rep["best_iteration"]))
    # the refine call's time on the last run, interleaved with the joint pose call
    tj, tf = [], []
    for i in range(reps + 1):
        a = timed(lambda: pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3))
        b = timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref3))
        if i:
            tj.append(a)
            tf.append(b)
    ok_j, ok_r = np.array(ok_j), np.array(ok_r)
    out["sizes"].append({"samples_per_run": total, "joint": rate(ok_j), "refined": rate(ok_r),
                         "fail_to_success": np.nonzero(~ok_j & ok_r)[0].tolist(),
                         "success_to_fail": np.nonzero(ok_j & ~ok_r)[0].tolist(),
                         "joint_verdicts": ok_j.astype(int).tolist(), "refined_verdicts": ok_r.astype(int).tolist(),
                         "median_rot21_rad": [med(res_j, 0), med(res_r, 0)],
                         "median_rot31_rad": [med(res_j, 1), med(res_r, 1)],
                         "median_joint_inliers": [int(np.median(cnt_j)), int(np.median(cnt_r))],
                         "joint_inliers": cnt_j, "refined_inliers": cnt_r,
                         "rot_residuals_joint": [[round(v, 5) for v in r[:2]] for r in res_j],
                         "rot_residuals_refined": [[round(v, 5) for v in r[:2]] for r in res_r],
                         "status": status, "best_iteration": best_it,
                         "joint_call_ms": summary(tj), "refine_call_ms": summary(tf)})
    del res, inl3
print(json.dumps(out))
