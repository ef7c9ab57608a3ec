#!/usr/bin/env python3
"""Early stop on noisy data: the gated abort launch against today's path on the
config-5 protocol (development tool, GPU).  Prints one JSON line.

Protocol of scripts/joint_pose.py: dataset 000 with sigma = 1 px noise, trial t
uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each budget
(300 and 1000 samples).  Per trial:
  (a) the plain tracking launch of the whole budget + hc_trifocal_pose_support_joint
      (today's path: abort mode's 0.90 gate never passes on this data);
  (b) for each ratio in RATIOS, with the reference's semantics and with
      inflight_stop: hc_trifocal_2op1p_30x30_track_abort_gated (T = 1) +
      hc_trifocal_pose_support_joint over what was tracked.
The verdict of each is hc_pose_residuals of the selected pose against the
ground truth.  Reported per budget, ratio and mode: successes with Wilson 95 %
intervals for (a) and (b), the trials whose verdict changed in each direction,
the trials that fired, the sample index of the firing path (the first passing
batch id), the paths tracked, and the time of (a) and (b): HIP events around
launch + pose call, every variant timed once per trial (a trial is a
repetition: the variants interleave within it), trial 0 run twice and its first
pass dropped; median [min, max] over the trials, in ms.

    python scripts/gated_stop.py [TRIALS]
    python scripts/gated_stop.py --existing [REPS]

--existing: the launches that existed before the gated one, timed on the loaded
build (HC_TRIFOCAL_LIB selects another build): config 2 (100 samples, plain
tracking) and the grouped abort launch (noisy trial 0, T = 1, 300 samples: runs
the whole budget; clean 000 / 099 / 050 / 001, 8 samples each).  Run
alternately on the parent's build and this one for the regression check.
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
from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch  # noqa: E402
from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker  # noqa: E402

BUDGETS = (300, 1000)
RATIOS = (0.20, 0.27, 0.30, 0.39)
SIGMA = 1.0
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def rate(ok):
    k = int(np.sum(ok))
    return {"successes": k, "success_rate": round(k / len(ok), 4), "success_rate_95ci": wilson95(k, len(ok))}


def existing(reps):
    problem = load_problem()
    tr = DeviceTracker(problem, dev)
    out = {"build_id": _abi.build_id(_abi.LIB_PATH), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"), "reps": reps}
    clean = {i: load_ransac_data(i) for i in (0, 99, 50, 1)}
    tgt, dif, _ = prepare_target_params(problem, clean[0], seed=0, num_samples=100)
    t, d = torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev)
    res = tr.allocate(100)

    def plain():
        tr.reset_tracks(res)
        return timed(lambda: tr.launch(t, d, res))
    batches = {"grouped_noisy_T1_300": TripletBatch(problem, [synthcurves.noisy(clean[0], SIGMA, synthcurves.DEFAULT_SEED)],
                                                    seeds=0, samples_per_triplet=300).to(dev),
               "grouped_clean_T4_8": TripletBatch(problem, [clean[0], clean[99], clean[50], clean[1]], seeds=0,
                                                  samples_per_triplet=8, edgel_counts=[None, None, 1000, None]).to(dev)}
    bufs = {k: tr.allocate_grouped(b) for k, b in batches.items()}

    def grouped(k):
        tr.reset_tracks(bufs[k])
        return timed(lambda: tr.launch_grouped(batches[k], bufs[k]))
    ms = {"config2_ms": [], **{k + "_ms": [] for k in batches}}
    for i in range(reps + 1):   # the three launches interleaved within a repetition, one warm-up
        row = {"config2_ms": plain(), **{k + "_ms": grouped(k) for k in batches}}
        if i:
            for k, v in row.items():
                ms[k].append(v)
    tr.workspace_status()
    out.update({k: summary(v) for k, v in ms.items()})
    out["grouped_found"] = {k: bufs[k].found.cpu().tolist() for k in batches}
    print(json.dumps(out))


def main(trials):
    problem = load_problem()
    data = load_ransac_data(0)
    tr = DeviceTracker(problem, dev)
    noisy = [synthcurves.noisy(data, SIGMA, synthcurves.DEFAULT_SEED + t) for t in range(trials)]
    E = data.locations.shape[0]
    variants = [(g, m) for g in RATIOS for m in (0, 1)]
    out = {"build_id": _abi.build_id(), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
           "workload": "config 5 protocol: Triplet_Edgels_000, sigma = %g px (noise seed 20250215 + trial), samples "
                       "srand(trial); (a) plain launch + joint pose support, (b) gated launch (T = 1) + joint pose "
                       "support over what was tracked" % SIGMA,
           "trials": trials, "edgels": E, "ratios": list(RATIOS), "budgets": []}
    for total in BUDGETS:
        n = total * 312
        res = tr.allocate(total, stats=False)
        inl = torch.empty((n, 3), dtype=torch.int32, device=dev)
        sel = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
        ok_a, ms_a = [], []
        rec = {v: dict(ok=[], ms=[], fired=[], fire_sample=[], tracked=[], fire_good=[]) for v in variants}
        for i, t in enumerate([0] + list(range(trials))):   # trial 0 twice: the first pass warms up and is dropped
            keep = i > 0
            nd = noisy[t]
            batch = TripletBatch(problem, [nd], seeds=t, samples_per_triplet=total).to(dev)
            rg = tr.allocate_grouped(batch, gate=True)

            def joint_of(tracks, conv):
                pose.launch_pose_support_joint(tracks, conv, batch.edgels, batch.K[0], inl, sel)

            tr.reset_tracks(res)
            ta = timed(lambda: (tr.launch(batch.target, batch.diff, res, num_samples=total),
                                joint_of(res.tracks, res.converge)))
            ja = pose.joint_selection_dict(pose.joint_selection_struct(sel))
            va = bool(pose.residuals(nd, ja)[1])
            if keep:
                ok_a.append(va)
                ms_a.append(ta)
            for g, m in variants:
                tr.reset_tracks(rg)
                tb = timed(lambda: (tr.launch_grouped(batch, rg, inflight_stop=bool(m), gate=g),
                                    joint_of(rg.tracks, rg.converge)))
                jb = pose.joint_selection_dict(pose.joint_selection_struct(sel))
                ids = torch.nonzero(rg.batch_index >= 0).reshape(-1)
                fired = int(rg.found[0].item()) != 0
                if not keep:
                    continue
                r = rec[(g, m)]
                r["ok"].append(bool(pose.residuals(nd, jb)[1]))
                r["ms"].append(tb)
                r["fired"].append(fired)
                r["fire_sample"].append(int(ids.min().item()) // 312 if fired else -1)
                r["tracked"].append(int((rg.stats[:, 0] > 0).sum().item()))
                # is the hypothesis that fired itself a success?  (scored alone)
                if fired:
                    only = torch.zeros_like(rg.converge)
                    only[ids.min()] = 1
                    joint_of(rg.tracks, only)
                    torch.cuda.synchronize(dev)
                    r["fire_good"].append(bool(pose.residuals(nd, pose.joint_selection_dict(
                        pose.joint_selection_struct(sel)))[1]))
            tr.workspace_status()
        ok_a = np.array(ok_a)
        b = {"samples_per_run": total, "paths_per_run": n, "plain": {**rate(ok_a), "ms": summary(ms_a),
                                                                    "verdicts": ok_a.astype(int).tolist()},
             "gated": []}
        for (g, m), r in rec.items():
            ok_b = np.array(r["ok"])
            b["gated"].append({"ratio": g, "min_joint_inliers": int(np.ceil(float(np.float32(g)) * E)),
                               "inflight_stop": m, **rate(ok_b),
                               "fail_to_success": np.nonzero(~ok_a & ok_b)[0].tolist(),
                               "success_to_fail": np.nonzero(ok_a & ~ok_b)[0].tolist(),
                               "fired": int(np.sum(r["fired"])), "fired_trials": np.nonzero(r["fired"])[0].tolist(),
                               "firing_hypothesis_good": int(np.sum(r["fire_good"])),
                               "fire_sample": r["fire_sample"],
                               "paths_tracked": {"median": int(np.median(r["tracked"])), "min": int(min(r["tracked"])),
                                                 "max": int(max(r["tracked"])), "per_trial": r["tracked"]},
                               "ms": summary(r["ms"]),
                               "ms_fired_trials": summary([x for x, f in zip(r["ms"], r["fired"]) if f]) if any(r["fired"]) else None,
                               "verdicts": ok_b.astype(int).tolist()})
        out["budgets"].append(b)
        del res, inl
    print(json.dumps(out))


if __name__ == "__main__":
    if "--existing" in sys.argv:
        a = [x for x in sys.argv[1:] if x != "--existing"]
        existing(int(a[0]) if a else 12)
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
