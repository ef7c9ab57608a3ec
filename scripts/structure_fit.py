#!/usr/bin/env python3
"""The structure stage on the config-5 protocol (development tool, GPU).
Prints one JSON line.

Protocol of scripts/threeview_fit.py: dataset 000 with sigma = 1 px noise, trial
t uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each of 100,
300 and 1000 samples.  In every run the device tracks are scored by the joint
call, the 8 best candidates are ranked, and hc_trifocal_pose_refine_topk refines
them through the three stages (10 iterations each, min_inliers 16, best by the
final transfer count) with the structure mode of
include/structure/hc_pose_structure.h, which reconstructs the 3D edgels of best.
Recorded per run: the GT verdict, the report's count, tangents and oriented, and
the median sin3 over the entries with a tangent.  Reported per size: the medians
of the three counts over the runs, and the median of the runs' median sin3 on
the runs that pass and on the runs that fail the GT check (no stage fits to the
tangents: the figure checks the pose on data it has not seen).  On the last run
the calls are timed by HIP events, interleaved within a repetition, REPS
repetitions after one warm-up (median, min, max in ms): refine_topk and
refine_joint in three-view mode and in structure mode, and the structure-only
call.

    python scripts/structure_fit.py [TRIALS [REPS]]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trifocal_pose_estimation_using_improved_gpuhc_amd import (_abi, load_problem, load_ransac_data, pose,  # noqa: E402
                                                               prepare_target_params, synthcurves)
from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker  # noqa: E402

SIZES = (100, 300, 1000)
K = 8
SIGMA = 1.0
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
trials = int(argv[0]) if len(argv) > 0 else 30
reps = int(argv[1]) if len(argv) > 1 else 12
dev = torch.device("cuda:0")
problem = load_problem()
data = load_ransac_data(0)
tr = DeviceTracker(problem, dev)
tangents = torch.from_numpy(np.ascontiguousarray(data.tangents)).to(dev)   # the noise moves the locations only


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


def med(v):
    return round(float(np.median(v)), 6) if len(v) else None


def run(nd, seed, total, res, inl3, sel3, cand):
    ta, da, _ = prepare_target_params(problem, nd, seed=seed, num_samples=total)
    tr.set_ransac_data(nd)
    tr.reset_tracks(res)
    tr.launch(torch.from_numpy(ta).to(dev), torch.from_numpy(da).to(dev), res, num_samples=total)
    pose.launch_pose_support_joint(res.tracks, res.converge, tr.edgels, tr.K, inl3, sel3)
    pose.launch_topk_joint(res.tracks, inl3, K, candidates=cand)


noisy = [synthcurves.noisy(data, SIGMA, synthcurves.DEFAULT_SEED + t) for t in range(trials)]
out = {"build_id": _abi.build_id(), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
       "workload": "config 5 protocol: Triplet_Edgels_000, sigma = %g px (noise seed 20250215 + trial), samples "
                   "srand(trial); the %d best joint candidates through the three stages (10 iterations each, "
                   "min_inliers 16), best by the final transfer count, and the 3D edgels of best (min_sin_plane and "
                   "max_sin3 0.05)" % (SIGMA, K),
       "trials": trials, "reps": reps, "k": K, "sizes": []}
for total in SIZES:
    res = tr.allocate(total, stats=False)
    inl3 = torch.empty((total * 312, 3), dtype=torch.int32, device=dev)
    sel3 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    cand = torch.empty(K * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    rows = []
    for t in range(trials):
        nd = noisy[t]
        run(nd, t, total, res, inl3, sel3, cand)
        o = pose.launch_refine_topk(cand, tr.edgels, tr.K, structure=True, tangents=tangents, select_by_transfer=True)
        torch.cuda.synchronize(dev)
        best = pose.joint_selection_dict(pose.joint_selection_struct(o[0]))
        rep = pose.structure_report_dict(o[7])
        rec = pose.structure_records(o[6], rep)
        has = (rec["flags"] & _abi.HC_EDGEL3D_TANGENT) != 0
        _, ok = pose.residuals(nd, best)
        rows.append(dict(ok=bool(ok), rank=int(o[1].cpu().numpy()[0]), status=rep["status"], count=rep["count"],
                         tangents=rep["tangents"], oriented=rep["oriented"],
                         median_sin3=float(np.median(rec["sin3"][has])) if has.any() else None))
    # the calls' times on the last run, interleaved
    ref1 = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    rec1 = torch.empty(int(tr.edgels.shape[0]) * pose.EDGEL3D_BYTES, dtype=torch.uint8, device=dev)
    st = dict(structure=True, tangents=tangents)
    calls = {"refine_topk_three_view": lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K, three_view=True),
             "refine_topk_structure": lambda: pose.launch_refine_topk(cand, tr.edgels, tr.K, **st),
             "refine_joint_three_view": lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1, three_view=True),
             "refine_joint_structure": lambda: pose.launch_refine_joint(sel3, tr.edgels, tr.K, out=ref1, edgels3d=rec1,
                                                                        **st),
             "reconstruct": lambda: pose.launch_reconstruct(o[0], tr.edgels, tangents, tr.K, out=ref1, edgels3d=rec1)}
    T = {k: [] for k in calls}
    for i in range(reps + 1):
        v = {k: timed(fn) for k, fn in calls.items()}
        if i:
            for k in T:
                T[k].append(v[k])
    ok = np.array([r["ok"] for r in rows])
    size = {"samples_per_run": total, "successes": int(ok.sum()), "call_ms": {k: summary(v) for k, v in T.items()},
            "count_median": med([r["count"] for r in rows]), "tangents_median": med([r["tangents"] for r in rows]),
            "oriented_median": med([r["oriented"] for r in rows]),
            "median_sin3_on_successes": med([r["median_sin3"] for r in rows if r["ok"] and r["median_sin3"] is not None]),
            "median_sin3_on_failures": med([r["median_sin3"] for r in rows if not r["ok"] and r["median_sin3"] is not None]),
            "runs": rows}
    out["sizes"].append(size)
    print(f"{total} samples: {int(ok.sum())}/{trials} pass, median count {size['count_median']}, oriented "
          f"{size['oriented_median']}, sin3 {size['median_sin3_on_successes']} | {size['median_sin3_on_failures']}",
          file=sys.stderr, flush=True)
    del res, inl3
print(json.dumps(out))
