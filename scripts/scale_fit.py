#!/usr/bin/env python3
"""The relative scale fitted by three-view transfer support, on the config-5
protocol (development tool, GPU).  Prints one JSON line.

Protocol of scripts/topk_refine.py: dataset 000 with sigma = 1 px noise, trial t
uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each of 100,
300 and 1000 samples.  In every run the device tracks are scored by the joint
call, the 8 best candidates are ranked, and hc_trifocal_pose_refine_topk
refines them (10 iterations, min_inliers 16) with the scale mode of
include/scale/hc_pose_scale.h, once selecting as before and once with
HC_SCALE_SELECT_BY_TRANSFER.  Recorded per run: the stored solver ratio of the
selected candidate, the fitted scale, transfer_inliers and the joint count, and
the GT verdict of both selections.  The true scale is not in the GT files
(they store unit translations): it is the vote on the noiseless edgels under
the GT poses.  Reported per size: the success rates with Wilson 95 % intervals,
the runs whose verdict changed, the fitted scale's relative error (median,
max) over the runs that pass the GT check, and the same for the solver ratio.
On the last run the calls are timed by HIP events, interleaved within a
repetition, REPS repetitions after one warm-up (median, min, max in ms):
refine_topk and refine_joint with the mode off and on, and the scale-only call.

    python scripts/scale_fit.py [TRIALS [REPS]]
    python scripts/scale_fit.py --existing     # the mode-off calls only, on the loaded build (HC_TRIFOCAL_LIB):
                                               # their times and a digest of their outputs, for an A/B of builds
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
                   "srand(trial); the %d best joint candidates refined (10 iterations, min_inliers 16), scale31 of "
                   "all fitted by three-view transfer support; best by joint count, and by transfer count" % (SIGMA, K),
       "trials": trials, "reps": reps, "k": K,
       "true_scale": {"scale31": true_scale, "transfer_inliers": gt_rep["transfer_inliers"], "tested": gt_rep["tested"],
                      "edgels": int(tr.edgels.shape[0])},
       "sizes": []}
for total in SIZES:
    res, inl3, sel3, cand = buffers(total)
    rows = {"joint": [], "transfer": []}
    for t in range(trials):
        nd = noisy[t]
        run(nd, t, total, res, inl3, sel3, cand)
        a = pose.launch_refine_topk(cand, tr.edgels, tr.K, fit_scale=True)
        b = pose.launch_refine_topk(cand, tr.edgels, tr.K, fit_scale=True, select_by_transfer=True)
        torch.cuda.synchronize(dev)
        ratios = [s["scale31"] for s in pose._selection_dicts(cand, K)]
        for name, o in (("joint", a), ("transfer", b)):
            rank = int(o[1].cpu().numpy()[0])
            best = pose.joint_selection_dict(pose.joint_selection_struct(o[0]))
            _, ok = pose.residuals(nd, best)
            sr = pose._scale_report_dicts(o[4], K)[rank] if rank >= 0 else None
            rows[name].append(dict(ok=bool(ok), rank=rank, path=int(best["path"]), joint=int(best["inliers"]),
                                   solver_ratio=float(ratios[rank]) if rank >= 0 else None,
                                   scale31=float(best["scale31"]),
                                   transfer_inliers=sr["transfer_inliers"] if sr else 0,
                                   tested=sr["tested"] if sr else 0, status=sr["status"] if sr else -1))
    # the calls' times on the last run, interleaved
    ref1 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    T = {k: [] for k in ("refine_topk", "refine_topk_fit", "refine_joint", "refine_joint_fit", "scale_only")}
    for i in range(reps + 1):
        v = {"refine_topk": timed(lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K)),
             "refine_topk_fit": timed(lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K, fit_scale=True)),
             "refine_joint": timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1)),
             "refine_joint_fit": timed(lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1,
                                                                        fit_scale=True)),
             "scale_only": timed(lambda: pose.launch_fit_scale31(ref1, tr.edgels, tr.K))}
        if i:
            for k in T:
                T[k].append(v[k])
    size = {"samples_per_run": total, "call_ms": {k: summary(v) for k, v in T.items()}}
    okj = np.array([r["ok"] for r in rows["joint"]])
    okt = np.array([r["ok"] for r in rows["transfer"]])
    for name, ok in (("joint", okj), ("transfer", okt)):
        good = [r for r in rows[name] if r["ok"]]
        size["select_by_" + name] = {
            **rate(ok), "verdicts": ok.astype(int).tolist(),
            "fitted_scale_rel_error_on_successes": spread([abs(r["scale31"] / true_scale - 1.0) for r in good]),
            "solver_ratio_rel_error_on_successes": spread([abs(r["solver_ratio"] / true_scale - 1.0) for r in good]),
            "runs": rows[name]}
    size["fail_to_success_by_transfer"] = np.nonzero(~okj & okt)[0].tolist()
    size["success_to_fail_by_transfer"] = np.nonzero(okj & ~okt)[0].tolist()
    out["sizes"].append(size)
    print(f"{total} samples: by joint {int(okj.sum())}/{trials}, by transfer {int(okt.sum())}/{trials}", file=sys.stderr,
          flush=True)
    del res, inl3
print(json.dumps(out))
