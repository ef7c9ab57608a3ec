#!/usr/bin/env python3
"""The refined joint winner against the best of the K refined top-K candidates,
on the config-5 protocol (development tool, GPU).  Prints one JSON line.

Protocol of scripts/refine_pose.py: dataset 000 with sigma = 1 px noise, trial t
uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each of 100,
300 and 1000 samples.  In every run the device tracks are scored once by
hc_trifocal_pose_support_joint; then for K = 1, 2, 4, 8, 16 on the same tracks
hc_trifocal_pose_topk_joint ranks the K best candidates and
hc_trifocal_pose_refine_topk refines them (10 iterations, min_inliers 16) and
selects; the verdict is hc_pose_residuals against the ground truth.  K = 1 is
the refined joint winner.  Reported per size and K: successes and rate with the
Wilson 95 % interval, the runs whose verdict changed against K = 1 in each
direction, the per-trial verdicts, the histogram of best_rank, the median joint
inliers; and on the last run the time of the top-k call (K = 8), of
refine_topk (K = 8) and of refine_joint beside them: HIP events, the calls
interleaved within a repetition, REPS repetitions after one warm-up; median,
min and max in ms.

    python scripts/topk_refine.py [TRIALS [REPS]]
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
KS = (1, 2, 4, 8, 16)
TIMED_K = 8
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
                   "srand(trial); the K best joint candidates refined (10 iterations, min_inliers 16) and the one "
                   "with the most joint inliers selected; K = 1 is the refined joint winner" % SIGMA,
       "trials": trials, "reps": reps, "ks": list(KS), "sizes": []}
for total in SIZES:
    res = tr.allocate(total, stats=False)
    n = total * 312
    inl3 = torch.empty((n, 3), dtype=torch.int32, device=dev)
    sel3 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    ref3 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    cand = {k: torch.empty(k * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev) for k in KS}
    ok = {k: [] for k in KS}
    ranks = {k: [] for k in KS}
    counts = {k: [] for k in KS}
    paths = {k: [] for k in KS}
    num_cand = []
    for t in range(trials):
        nd = noisy[t]
        ta, da, _ = prepare_target_params(problem, nd, seed=t, num_samples=total)
        tr.set_ransac_data(nd)
        tr.reset_tracks(res)
        tr.launch(torch.from_numpy(ta).to(dev), torch.from_numpy(da).to(dev), res, num_samples=total)
        pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3)
        outs = {}
        for k in KS:
            pose.launch_topk_joint(res.tracks, inl3, k, candidates=cand[k])
            outs[k] = pose.launch_refine_topk(cand[k], tr.edgels, tr.K)
        torch.cuda.synchronize(dev)
        j = pose.joint_selection_dict(pose.joint_selection_struct(sel3))
        num_cand.append(int(j["num_candidates"]))
        for k in KS:
            best, best_rank = outs[k][0], int(outs[k][1].cpu().numpy()[0])
            b = pose.joint_selection_dict(pose.joint_selection_struct(best))
            assert cand[k][:pose.JOINT_SEL_BYTES].cpu().numpy().tobytes() == sel3.cpu().numpy().tobytes()
            _, okb = pose.residuals(nd, b)
            ok[k].append(bool(okb))
            ranks[k].append(best_rank)
            counts[k].append(int(b["inliers"]))
            paths[k].append(int(b["path"]))
    # the calls' times on the last run, interleaved
    tt, tk, t1 = [], [], []
    for i in range(reps + 1):
        a = timed(lambda: pose.launch_topk_joint(res.tracks, inl3, TIMED_K, candidates=cand[TIMED_K]))
        b = timed(lambda: pose.launch_refine_topk(cand[TIMED_K], tr.edgels, tr.K))
        c = timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref3))
        if i:
            tt.append(a)
            tk.append(b)
            t1.append(c)
    base = np.array(ok[1])
    per_k = []
    for k in KS:
        o = np.array(ok[k])
        hist = {str(r): int(np.sum(np.array(ranks[k]) == r)) for r in sorted(set(ranks[k]))}
        per_k.append({"k": k, **rate(o), "fail_to_success_vs_k1": np.nonzero(~base & o)[0].tolist(),
                      "success_to_fail_vs_k1": np.nonzero(base & ~o)[0].tolist(), "verdicts": o.astype(int).tolist(),
                      "best_rank_histogram": hist, "best_rank": ranks[k],
                      "median_joint_inliers": int(np.median(counts[k])), "joint_inliers": counts[k], "path": paths[k]})
    out["sizes"].append({"samples_per_run": total, "num_candidates": num_cand, "per_k": per_k,
                         "topk_call_ms": summary(tt), "refine_topk_call_ms": summary(tk),
                         "refine_joint_call_ms": summary(t1), "timed_k": TIMED_K})
    print(f"{total} samples: " + ", ".join(f"K={p['k']} {p['successes']}/{trials}" for p in per_k), file=sys.stderr,
          flush=True)
    del res, inl3
print(json.dumps(out))
