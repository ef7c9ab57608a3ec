#!/usr/bin/env python3
"""The adaptive sample limit against a fixed budget and against the ratio gate,
on the config-5 protocol (development tool, GPU).  Prints one JSON line.

Protocol of scripts/gated_stop.py: dataset 000 with sigma = 1 px noise, trial t
uses noise seed 20250215 + t and samples srand(t); TRIALS runs at each budget
(300 and 1000 samples).  Per trial, every variant tracks from the start
solutions and is timed once (HIP events around launch + pose call; a trial is a
repetition and the variants interleave within it; trial 0 is run twice and its
first pass dropped):
  plain            the plain launch of the whole budget + hc_trifocal_pose_support_joint
  gate_0.39        the gated launch at ratio 0.39 + joint support over what was tracked
  adaptive_p0.99   the gated launch's adaptive mode, confidence 0.99, ratio off
  adaptive_p0.999  the same at confidence 0.999
  adaptive_p0.99_inflight   confidence 0.99 with inflight_stop
  plain_topk       the plain launch + pose.select_refined (k = 8)
  adaptive_topk    adaptive 0.99 + pose.select_refined (k = 8) over what was tracked
The verdict of each is hc_pose_residuals of the selected pose against the ground
truth.  Per budget and variant: successes with the Wilson 95 % interval, the
trials whose verdict changed in each direction against `plain` (the two top-k
rows also against each other), the final limit and the paths tracked per trial,
and the time as median [min, max] over the trials, in ms.

    python scripts/adaptive_stop.py [TRIALS]
    python scripts/adaptive_stop.py --existing [REPS]

--existing: launches that existed before the adaptive mode, timed on the loaded
build (HC_TRIFOCAL_LIB selects another build, e.g. the parent's): config 2 (100
samples, plain tracking), one sample, and the gated launch at ratio 0.39 on the
noisy trial 0 with 300 samples (T = 1); interleaved within a repetition, one
warm-up.  Run alternately on the parent's build and this one.
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
GATE = 0.39
SIGMA = 1.0
TOPK = 8
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
    clean = load_ransac_data(0)
    tgt, dif, _ = prepare_target_params(problem, clean, seed=0, num_samples=100)
    t, d = torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev)
    res = {n: tr.allocate(n) for n in (100, 1)}
    batch = TripletBatch(problem, [synthcurves.noisy(clean, SIGMA, synthcurves.DEFAULT_SEED)], seeds=0,
                         samples_per_triplet=300).to(dev)
    rg = tr.allocate_grouped(batch, gate=True)

    def plain(n):
        tr.reset_tracks(res[n])
        return timed(lambda: tr.launch(t, d, res[n], num_samples=n))

    def gated():
        tr.reset_tracks(rg)
        return timed(lambda: tr.launch_grouped(batch, rg, gate=GATE))
    ms = {"config2_ms": [], "one_sample_ms": [], "gated_noisy_T1_300_ms": []}
    for i in range(reps + 1):
        row = {"config2_ms": plain(100), "one_sample_ms": plain(1), "gated_noisy_T1_300_ms": gated()}
        if i:
            for k, v in row.items():
                ms[k].append(v)
    tr.workspace_status()
    out.update({k: summary(v) for k, v in ms.items()})
    out["gated_found"] = rg.found.cpu().tolist()
    out["gated_paths_tracked"] = int((rg.stats[:, 0] > 0).sum().item())
    print(json.dumps(out))


def main(trials):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import AdaptiveStop
    problem = load_problem()
    data = load_ransac_data(0)
    tr = DeviceTracker(problem, dev)
    noisy = [synthcurves.noisy(data, SIGMA, synthcurves.DEFAULT_SEED + t) for t in range(trials)]
    E = data.locations.shape[0]
    # name -> (launch keywords or None for the plain launch, top-k refinement after it)
    variants = {"plain": (None, False),
                "gate_%.2f" % GATE: (dict(gate=GATE), False),
                "adaptive_p0.99": (dict(adaptive=AdaptiveStop(0.99)), False),
                "adaptive_p0.999": (dict(adaptive=AdaptiveStop(0.999)), False),
                "adaptive_p0.99_inflight": (dict(adaptive=AdaptiveStop(0.99), inflight_stop=True), False),
                "plain_topk": (None, True),
                "adaptive_topk": (dict(adaptive=AdaptiveStop(0.99)), True)}
    out = {"build_id": _abi.build_id(), "measured_at": time.strftime("%Y-%m-%dT%H:%M:%S"),
           "workload": "config 5 protocol: Triplet_Edgels_000, sigma = %g px (noise seed 20250215 + trial), samples "
                       "srand(trial); every variant tracks from the start solutions, then joint pose support (or "
                       "select_refined, k = %d) over what was tracked" % (SIGMA, TOPK),
           "trials": trials, "edgels": E, "gate": GATE, "topk": TOPK, "budgets": []}
    for total in BUDGETS:
        n = total * 312
        res = tr.allocate(total, stats=True)
        inl = torch.empty((n, 3), dtype=torch.int32, device=dev)
        sel = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
        rec = {v: dict(ok=[], ms=[], limit=[], tracked=[], fired=[]) for v in variants}
        for i, t in enumerate([0] + list(range(trials))):   # trial 0 twice: the first pass warms up and is dropped
            nd = noisy[t]
            batch = TripletBatch(problem, [nd], seeds=t, samples_per_triplet=total).to(dev)
            rg = tr.allocate_grouped(batch, adaptive=True)
            for name, (kw, topk) in variants.items():
                r = res if kw is None else rg
                tr.reset_tracks(r)
                if kw is not None:
                    rg.limit.fill_(total)
                    if "adaptive" in kw:
                        kw["adaptive"].prepare(batch)   # the tables' device copies: not part of the timed launch
                best = {}

                def run():
                    if kw is None:
                        tr.launch(batch.target, batch.diff, res, num_samples=total)
                    else:
                        tr.launch_grouped(batch, rg, **kw)
                    if topk:
                        best["sel"] = pose.select_refined(r.tracks, r.converge, batch.edgels, batch.K[0], k=TOPK)[0]
                    else:
                        pose.launch_pose_support_joint(r.tracks, r.converge, batch.edgels, batch.K[0], inl, sel)
                ms = timed(run)
                chosen = best["sel"] if topk else pose.joint_selection_dict(pose.joint_selection_struct(sel))
                if i == 0:
                    continue
                q = rec[name]
                q["ok"].append(bool(pose.residuals(nd, chosen)[1]))
                q["ms"].append(ms)
                q["tracked"].append(int((r.stats[:, 0] > 0).sum().item()))
                q["limit"].append(int(rg.limit[0].item()) if kw is not None and "adaptive" in kw else total)
                q["fired"].append(bool(kw is not None and int(rg.found[0].item()) != 0))
            tr.workspace_status()
        base = np.array(rec["plain"]["ok"])
        rows = []
        for name, q in rec.items():
            ok = np.array(q["ok"])
            row = {"variant": name, **rate(ok), "fail_to_success": np.nonzero(~base & ok)[0].tolist(),
                   "success_to_fail": np.nonzero(base & ~ok)[0].tolist(),
                   "final_limit": {"median": int(np.median(q["limit"])), "min": int(min(q["limit"])),
                                   "max": int(max(q["limit"])), "per_trial": q["limit"]},
                   "paths_tracked": {"median": int(np.median(q["tracked"])), "min": int(min(q["tracked"])),
                                     "max": int(max(q["tracked"])), "per_trial": q["tracked"]},
                   "fired": int(np.sum(q["fired"])), "ms": summary(q["ms"]), "verdicts": ok.astype(int).tolist()}
            if name == "adaptive_topk":
                ref = np.array(rec["plain_topk"]["ok"])
                row["fail_to_success_vs_plain_topk"] = np.nonzero(~ref & ok)[0].tolist()
                row["success_to_fail_vs_plain_topk"] = np.nonzero(ref & ~ok)[0].tolist()
            rows.append(row)
        out["budgets"].append({"samples_per_run": total, "paths_per_run": n, "variants": rows})
        print(f"{total} samples: " + ", ".join(f"{r['variant']} {r['successes']}/{trials} {r['ms']['median']} ms"
                                               for r in rows), file=sys.stderr, flush=True)
        del res, inl
    print(json.dumps(out))


if __name__ == "__main__":
    if "--existing" in sys.argv:
        a = [x for x in sys.argv[1:] if x != "--existing"]
        existing(int(a[0]) if a else 12)
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
