#!/usr/bin/env python3
"""Per-view against joint pose selection on the config-5 protocol (development
tool, GPU).  Prints one JSON line.

Protocol of bench.py's noisy_pose leg: dataset 000 with sigma = 1 px noise,
trial t uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each
of 100, 300 and 1000 samples.  In every run the same device tracks are scored
by hc_trifocal_pose_support (views selected independently) and by
hc_trifocal_pose_support_joint (one hypothesis, most edgels within 2 px in both
views); the verdict of each is hc_pose_residuals against the ground truth.
Reported per size: successes and rate with the Wilson 95 % interval for each
rule, the runs whose verdict changed in each direction, the per-trial verdicts,
and the time of each pose call on the last run's tracks: HIP events, the two
calls interleaved within a repetition, REPS repetitions after one warm-up;
median, min and max in ms.

    python scripts/joint_pose.py [TRIALS [REPS]]
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


out = {"build_id": _abi.build_id(), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
       "workload": "config 5 protocol: Triplet_Edgels_000, sigma = %g px (noise seed 20250215 + trial), samples "
                   "srand(trial); both selections on the same device tracks" % SIGMA,
       "trials": trials, "reps": reps, "sizes": []}
for total in SIZES:
    res = tr.allocate(total, stats=False)
    n = total * 312
    inl2 = torch.empty((n, 2), dtype=torch.int32, device=dev)
    sel2 = torch.empty(pose.SEL_BYTES, dtype=torch.uint8, device=dev)
    inl3 = torch.empty((n, 3), dtype=torch.int32, device=dev)
    sel3 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    ok_v, ok_j, same_path, joint_counts, cands = [], [], [], [], []
    for t in range(trials):
        nd = noisy[t]
        ta, da, _ = prepare_target_params(problem, nd, seed=t, num_samples=total)
        tr.set_ransac_data(nd)
        tr.reset_tracks(res)
        tr.launch(torch.from_numpy(ta).to(dev), torch.from_numpy(da).to(dev), res, num_samples=total)
        pose.launch_pose_support(res.tracks, res.converge, tr.edgels, tr.K, inl2, sel2)
        pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3)
        torch.cuda.synchronize(dev)
        v = pose.selection_dict(pose.selection_struct(sel2))
        j = pose.joint_selection_dict(pose.joint_selection_struct(sel3))
        # the joint call's per-view counts are the per-view call's
        assert torch.equal(inl3[:, 1:], inl2) and v["num_candidates"] == j["num_candidates"]
        ok_v.append(bool(pose.residuals(nd, v)[1]))
        ok_j.append(bool(pose.residuals(nd, j)[1]))
        same_path.append(bool(v["path21"] == v["path31"]))
        joint_counts.append(int(j["inliers"]))
        cands.append(int(j["num_candidates"]))
    # pose-call time on the last run's tracks, the two calls interleaved
    tv, tj = [], []
    for i in range(reps + 1):
        a = timed(lambda: pose.launch_pose_support(res.tracks, res.converge, tr.edgels, tr.K, inl2, sel2))
        b = timed(lambda: pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3))
        if i:
            tv.append(a)
            tj.append(b)
    ok_v, ok_j = np.array(ok_v), np.array(ok_j)
    out["sizes"].append({"samples_per_run": total, "per_view": rate(ok_v), "joint": rate(ok_j),
                         "fail_to_success": np.nonzero(~ok_v & ok_j)[0].tolist(),
                         "success_to_fail": np.nonzero(ok_v & ~ok_j)[0].tolist(),
                         "per_view_verdicts": ok_v.astype(int).tolist(), "joint_verdicts": ok_j.astype(int).tolist(),
                         "per_view_same_path_runs": int(np.sum(same_path)),
                         "median_candidates": int(np.median(cands)),
                         "median_joint_inliers": int(np.median(joint_counts)),
                         "pose_call_candidates": cands[-1],
                         "per_view_call_ms": summary(tv), "joint_call_ms": summary(tj)})
    del res, inl2, inl3
print(json.dumps(out))
