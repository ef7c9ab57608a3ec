#!/usr/bin/env python3
"""Several triplets: T sequential single-triplet runs against one grouped run
(development tool, GPU).  Prints one JSON line.

(a) sequential: per triplet, track(abort) on its 8 samples, then pose_support,
    each triplet on the tracker's one workspace, stream-ordered, no host sync
    in between (the favourable case for the sequential caller);
(b) grouped: one hc_trifocal_2op1p_30x30_track_abort_grouped launch over all
    the samples (triplet-major) and one hc_trifocal_pose_support_grouped call.
T in {1, 4, 16} triplets cycling the seven committed datasets, 8 samples each,
srand(0).  Also T = 1, dataset 000, 1000 samples: the grouped launch against
the existing abort launch (tracking only).  Timing: HIP events around each
variant's enqueues, the variants interleaved within a repetition, REPS
repetitions after one warm-up; median, min and max in ms.

    python scripts/multi_triplet.py [REPS]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, load_problem, load_ransac_data, pose  # noqa
from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch  # noqa
from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker  # noqa

DATASETS = (0, 1, 2, 3, 10, 50, 99)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
dev = torch.device("cuda:0")
problem = load_problem()
datas = {i: load_ransac_data(i) for i in DATASETS}
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


class Sequential:
    """One triplet's own buffers for the single-triplet entry points."""

    def __init__(self, batch, db, t):
        rows = torch.from_numpy(batch.index[t]).to(dev)
        self.target, self.diff = db.target[rows].contiguous(), db.diff[rows].contiguous()
        self.edgels, self.K = db.group_edgels(t), db.K[t]
        self.r = tr.allocate(len(batch.index[t]), stats=True, abort=True)
        n = self.r.converge.numel()
        self.inl = torch.empty((n, 2), dtype=torch.int32, device=dev)
        self.sel = torch.empty(pose.SEL_BYTES, dtype=torch.uint8, device=dev)

    def reset(self):
        tr.reset_tracks(self.r)

    def run(self, with_pose=True):
        tr.edgels, tr.K = self.edgels, self.K
        tr.launch(self.target, self.diff, self.r, abort=True)
        if with_pose:
            pose.launch_pose_support(self.r.tracks, self.r.converge, self.edgels, self.K, self.inl, self.sel)


class Grouped:
    def __init__(self, db):
        self.db = db
        self.r = tr.allocate_grouped(db)
        n = self.r.converge.numel()
        self.inl = torch.empty((n, 2), dtype=torch.int32, device=dev)
        self.sel = torch.empty(db.num_groups * pose.SEL_BYTES, dtype=torch.uint8, device=dev)

    def reset(self):
        tr.reset_tracks(self.r)

    def run(self, with_pose=True):
        tr.launch_grouped(self.db, self.r)
        if with_pose:
            pose.launch_pose_support_grouped(self.r.tracks, self.r.converge, self.db, self.inl, self.sel)


def compare(batch, with_pose):
    db = batch.to(dev)
    seq = [Sequential(batch, db, t) for t in range(batch.num_groups)]
    grp = Grouped(db)
    ts, tg = [], []
    for i in range(reps + 1):
        for s in seq:
            s.reset()
        grp.reset()
        a = timed(lambda: [s.run(with_pose) for s in seq])
        b = timed(lambda: grp.run(with_pose))
        if i:
            ts.append(a)
            tg.append(b)
    # the two variants found for the same triplets
    f_seq = [int(s.r.found.item()) for s in seq]
    f_grp = [int(v != 0) for v in grp.r.found.cpu().tolist()]
    assert f_seq == f_grp, (f_seq, f_grp)
    return {"sequential_ms": summary(ts), "grouped_ms": summary(tg),
            "ratio_median": round(float(np.median(tg) / np.median(ts)), 4), "found": f_grp}


out = {"build": _abi.build_id(), "reps": reps, "samples_per_triplet": 8, "triplets": {}}
for T in (1, 4, 16):
    ds = [datas[DATASETS[i % len(DATASETS)]] for i in range(T)]
    out["triplets"][str(T)] = compare(TripletBatch(problem, ds, seeds=0, samples_per_triplet=8), True)
out["single_triplet_1000_samples"] = compare(TripletBatch(problem, [datas[0]], seeds=0, samples_per_triplet=1000), False)
print(json.dumps(out))
