#!/usr/bin/env python3
"""The three-view refinement on the config-5 protocol (development tool, GPU).
Prints one JSON line.

Protocol of scripts/scale_fit.py: dataset 000 with sigma = 1 px noise, trial t
uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each of 100,
300 and 1000 samples.  In every run the device tracks are scored by the joint
call, the 8 best candidates are ranked, and hc_trifocal_pose_refine_topk refines
them (10 iterations, min_inliers 16) once with the scale mode of
include/scale/hc_pose_scale.h ("without": the two-view refinement and the voted
scale) and once with the three-view mode of include/threeview/hc_pose_threeview.h
("with": ten more steps on both views and the scale jointly), both selecting by
the final transfer count.  Recorded per run and mode: the GT verdict, the two
rotation residuals, the scale's relative error against the true scale (the vote
on the noiseless edgels under the GT poses) and the final transfer inliers.
Reported per size: the success counts with the runs whose verdict changed in
either direction, and the median and maximum of the rotation residuals and of
the scale error over the runs that pass the GT check.  On the last run the calls
are timed by HIP events, interleaved within a repetition, REPS repetitions after
one warm-up (median, min, max in ms): refine_topk and refine_joint without and
with the stage.

    python scripts/threeview_fit.py [TRIALS [REPS]]
    python scripts/threeview_fit.py --existing   # the mode-off calls only, on the loaded build (HC_TRIFOCAL_LIB):
                                                 # refine_joint and refine_topk on trial 0 at 100 samples, their
                                                 # times and a digest of their outputs, for an A/B of builds
"""
import hashlib
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
K = 8
SIGMA = 1.0
existing = "--existing" in sys.argv
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
trials = int(argv[0]) if len(argv) > 0 else 30
reps = int(argv[1]) if len(argv) > 1 else 12
dev = torch.device("cuda:0")
problem = load_problem()
data = load_ransac_data(0)
tr = DeviceTracker(problem, dev)


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


def spread(v):
    return {"median": round(float(np.median(v)), 6), "max": round(float(np.max(v)), 6)} if len(v) else None


def run(nd, seed, total, res, inl3, sel3, cand):
    ta, da, _ = prepare_target_params(problem, nd, seed=seed, num_samples=total)
    tr.set_ransac_data(nd)
    tr.reset_tracks(res)
    tr.launch(torch.from_numpy(ta).to(dev), torch.from_numpy(da).to(dev), res, num_samples=total)
    pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3)
    pose.launch_topk_joint(res.tracks, inl3, K, candidates=cand)


def buffers(total):
    return (tr.allocate(total, stats=False), torch.empty((total * 312, 3), dtype=torch.int32, device=dev),
            torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev),
            torch.empty(K * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev))


if existing:
    # the calls that existed before the mode, on trial 0 at 100 samples
    res, inl3, sel3, cand = buffers(100)
    run(synthcurves.noisy(data, SIGMA, synthcurves.DEFAULT_SEED), 0, 100, res, inl3, sel3, cand)
    ref1 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    tk, t1 = [], []
    for i in range(reps + 1):
        b = timed(lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K))
        c = timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1))
        if i:
            tk.append(b)
            t1.append(c)
    outs = pose.launch_refine_topk(cand, tr.edgels, tr.K) + pose.launch_refine_joint(sel3, tr.edgels, tr.K)
    torch.cuda.synchronize(dev)
    digest = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in outs)).hexdigest()[:16]
    print(json.dumps({"build_id": _abi.build_id(), "reps": reps, "refine_topk_call_ms": summary(tk),
                      "refine_joint_call_ms": summary(t1), "outputs_sha256": digest}))
    sys.exit(0)

# the true scale: the vote on the noiseless edgels under the GT poses
gt = _abi.hcTrifocalSelection()
gt.path, gt.num_candidates = 0, 1
gt.R21[:], gt.R31[:] = [float(v) for v in data.pose21[:9]], [float(v) for v in data.pose31[:9]]
for name, p in (("t21", data.pose21), ("t31", data.pose31)):
    t = np.asarray(p[9:], np.float64)
    getattr(gt, name)[:] = [float(v) for v in (t / np.linalg.norm(t)).astype(np.float32)]
tr.set_ransac_data(data)
_, gt_rep = pose.fit_scale31(gt, tr.edgels, tr.K)
true_scale = float(gt_rep["scale31"])

noisy = [synthcurves.noisy(data, SIGMA, synthcurves.DEFAULT_SEED + t) for t in range(trials)]
out = {"build_id": _abi.build_id(), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
       "workload": "config 5 protocol: Triplet_Edgels_000, sigma = %g px (noise seed 20250215 + trial), samples "
                   "srand(trial); the %d best joint candidates refined (10 iterations, min_inliers 16) and their scale "
                   "voted, without and with the three-view refinement (10 iterations); best by the final transfer "
                   "count" % (SIGMA, K),
       "trials": trials, "reps": reps, "k": K, "true_scale": true_scale, "sizes": []}
for total in SIZES:
    res, inl3, sel3, cand = buffers(total)
    rows = {"without": [], "with": []}
    for t in range(trials):
        nd = noisy[t]
        run(nd, t, total, res, inl3, sel3, cand)
        a = pose.launch_refine_topk(cand, tr.edgels, tr.K, fit_scale=True, select_by_transfer=True)
        b = pose.launch_refine_topk(cand, tr.edgels, tr.K, three_view=True, select_by_transfer=True)
        torch.cuda.synchronize(dev)
        for name, o in (("without", a), ("with", b)):
            rank = int(o[1].cpu().numpy()[0])
            best = pose.joint_selection_dict(pose.joint_selection_struct(o[0]))
            r4, ok = pose.residuals(nd, best)
            row = dict(ok=bool(ok), rank=rank, path=int(best["path"]), joint=int(best["inliers"]),
                       rot21=float(r4[0]), rot31=float(r4[1]), scale31=float(best["scale31"]))
            if rank < 0:
                row.update(transfer_inliers=0)
            elif name == "without":
                row.update(transfer_inliers=pose._scale_report_dicts(o[4], K)[rank]["transfer_inliers"])
            else:
                tv = pose._three_view_report_dicts(o[5], K)[rank]
                row.update(transfer_inliers=tv["transfer_inliers"], status=tv["status"],
                           best_iteration=tv["best_iteration"], fit_set=tv["fit_set"])
            rows[name].append(row)
    # the calls' times on the last run, interleaved
    ref1 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    T = {k: [] for k in ("refine_topk_fit", "refine_topk_three_view", "refine_joint_fit", "refine_joint_three_view")}
    for i in range(reps + 1):
        v = {"refine_topk_fit": timed(lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K, fit_scale=True)),
             "refine_topk_three_view": timed(lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K, three_view=True)),
             "refine_joint_fit": timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1,
                                                                        fit_scale=True)),
             "refine_joint_three_view": timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1,
                                                                               three_view=True))}
        if i:
            for k in T:
                T[k].append(v[k])
    size = {"samples_per_run": total, "call_ms": {k: summary(v) for k, v in T.items()}}
    okw = np.array([r["ok"] for r in rows["without"]])
    okt = np.array([r["ok"] for r in rows["with"]])
    for name, ok in (("without", okw), ("with", okt)):
        good = [r for r in rows[name] if r["ok"]]
        size[name] = {**rate(ok), "verdicts": ok.astype(int).tolist(),
                      "rot21_on_successes": spread([r["rot21"] for r in good]),
                      "rot31_on_successes": spread([r["rot31"] for r in good]),
                      "scale_rel_error_on_successes": spread([abs(r["scale31"] / true_scale - 1.0) for r in good]),
                      "transfer_inliers_on_successes": spread([r["transfer_inliers"] for r in good]),
                      "runs": rows[name]}
    size["fail_to_success"] = np.nonzero(~okw & okt)[0].tolist()
    size["success_to_fail"] = np.nonzero(okw & ~okt)[0].tolist()
    out["sizes"].append(size)
    print(f"{total} samples: without {int(okw.sum())}/{trials}, with {int(okt.sum())}/{trials}", file=sys.stderr,
          flush=True)
    del res, inl3
print(json.dumps(out))
