"""Several image triplets in one launch (grouped abort tracking, grouped pose support).

A caller with T triplets and a modest RANSAC budget each pays T small,
latency-bound launches with the single-triplet entry points.  The grouped ones
(include/hc_trifocal.h hc_trifocal_2op1p_30x30_track_abort_grouped,
include/hc_pose.h hc_trifocal_pose_support_grouped) take all the samples at
once: every sample carries the id of its triplet, and the scoring set, K, the
found flag and the selection are those of the sample's own triplet.

TripletBatch draws the samples and lays them out; DeviceTripletBatch holds the
device copies and the hcTripletGroup descriptor array.  check_groups is the
host-side validation every grouped launch goes through (the kernels do not
validate group ids).
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .problem import Problem, RansacData, prepare_target_params

GROUP_DTYPE = np.dtype([("locations", "<u8"), ("K", "<u8"), ("num_edgels", "<i4"), ("pad", "<i4")])
assert GROUP_DTYPE.itemsize == _abi.TRIPLET_GROUP_BYTES


def check_groups(sample_group, num_groups: int, num_samples: int, edgel_counts) -> None:
    """Raises HCError unless sample_group holds num_samples ids in
    [0, num_groups) and every one of the num_groups edgel counts is positive."""
    if int(num_groups) < 1:
        raise _abi.HCError(f"grouped launch: {num_groups} groups (at least one is needed)")
    sg = np.asarray(sample_group)
    if sg.ndim != 1 or sg.shape[0] != int(num_samples):
        raise _abi.HCError(f"grouped launch: sample_group has shape {sg.shape}, the launch {num_samples} samples")
    if sg.size and not np.issubdtype(sg.dtype, np.integer):
        raise _abi.HCError("grouped launch: sample_group must hold integers")
    if sg.size and (int(sg.min()) < 0 or int(sg.max()) >= int(num_groups)):
        bad = int(np.nonzero((sg < 0) | (sg >= int(num_groups)))[0][0])
        raise _abi.HCError(f"grouped launch: sample {bad} has group id {int(sg[bad])}, outside [0, {num_groups})")
    ec = np.asarray(edgel_counts)
    if ec.ndim != 1 or ec.shape[0] != int(num_groups):
        raise _abi.HCError(f"grouped launch: {ec.shape} edgel counts for {num_groups} groups")
    if (ec <= 0).any():
        bad = int(np.nonzero(ec <= 0)[0][0])
        raise _abi.HCError(f"grouped launch: group {bad} has {int(ec[bad])} edgels (must be positive)")


def _per_triplet(v, n: int, what: str) -> list:
    if np.isscalar(v) or v is None:
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise _abi.HCError(f"TripletBatch: {len(v)} {what} for {n} triplets")
    return v


class TripletBatch:
    """The samples of several triplets as one launch's inputs (host side).

    datas: one RansacData per triplet.  seeds / samples_per_triplet: one value
    for all or one per triplet; each triplet's samples are drawn by
    prepare_target_params from its full edgel set, as a single-triplet run
    draws them.  edgel_counts (optional, per triplet, None = all): the scoring
    set is the first that many edgels.  Order: triplet-major, or with
    interleave=True round-robin (sample 0 of every triplet, then sample 1, ...).

    target, diff (N, 34, 2), picked (N, 3): the concatenated rows;
    sample_group (N,) int32; index[t]: the rows of triplet t, in its own order;
    sample_ordinal (N,) int32: a row's index among its own triplet's rows, in
    launch order (the adaptive sample limit compares it with the triplet's limit).
    tangents[t]: the tangents of triplet t's scoring set, the first E rows of
    its data's (E, 6), beside locations[t] (the structure stage reads them).
    """

    def __init__(self, problem: Problem, datas, seeds=0, samples_per_triplet=8, interleave: bool = False,
                 edgel_counts=None):
        datas = list(datas)
        T = len(datas)
        if T < 1:
            raise _abi.HCError("TripletBatch: no triplets")
        seeds = _per_triplet(seeds, T, "seeds")
        counts = [int(c) for c in _per_triplet(samples_per_triplet, T, "sample counts")]
        if min(counts) < 0:
            raise _abi.HCError("TripletBatch: negative sample count")
        ecs = _per_triplet(edgel_counts, T, "edgel counts")
        self.datas = datas
        self.num_groups = T
        self.locations, self.Ks, self.tangents = [], [], []
        for t, (d, e) in enumerate(zip(datas, ecs)):
            E = d.locations.shape[0] if e is None else int(e)
            if E <= 0 or E > d.locations.shape[0]:
                raise _abi.HCError(f"TripletBatch: triplet {t}: scoring set of {E} of {d.locations.shape[0]} edgels")
            self.locations.append(np.ascontiguousarray(d.locations[:E], np.float32))
            self.tangents.append(np.ascontiguousarray(d.tangents[:E], np.float32))
            self.Ks.append(np.ascontiguousarray(d.K, np.float32).reshape(9))
        self.edgel_counts = np.array([l.shape[0] for l in self.locations], np.int32)
        parts = [prepare_target_params(problem, d, seed=int(s), num_samples=c) if c > 0 else
                 (np.zeros((0, 34, 2), np.float32), np.zeros((0, 34, 2), np.float32), np.zeros((0, 3), np.int32))
                 for d, s, c in zip(datas, seeds, counts)]
        if interleave:
            order = [(k, t) for k in range(max(counts)) for t in range(T) if k < counts[t]]
        else:
            order = [(k, t) for t in range(T) for k in range(counts[t])]
        self.num_samples = len(order)
        self.sample_group = np.array([t for _, t in order], np.int32)
        self.sample_ordinal = np.array([k for k, _ in order], np.int32)
        self.target = np.ascontiguousarray(np.stack([parts[t][0][k] for k, t in order])) if order else parts[0][0]
        self.diff = np.ascontiguousarray(np.stack([parts[t][1][k] for k, t in order])) if order else parts[0][1]
        self.picked = np.ascontiguousarray(np.stack([parts[t][2][k] for k, t in order])) if order else parts[0][2]
        self.index = [np.nonzero(self.sample_group == t)[0] for t in range(T)]
        check_groups(self.sample_group, T, self.num_samples, self.edgel_counts)

    def path_index(self, t: int) -> np.ndarray:
        """Batch ids (sample * 312 + track) of triplet t's paths, in its own order."""
        return (self.index[t][:, None] * _abi.NUM_TRACKS + np.arange(_abi.NUM_TRACKS)[None, :]).reshape(-1)

    def to(self, device) -> "DeviceTripletBatch":
        return DeviceTripletBatch(self, device)


class DeviceTripletBatch:
    """Device copies of a TripletBatch: target, diff, the concatenated edgels
    (sum E, 6), K (T, 9), sample_group and sample_ordinal (N,) int32 and `groups`, the
    hcTripletGroup array (T x 24 bytes) whose pointers go into edgels / K.
    tangents (sum E, 6) is laid out as edgels; edgel_offsets (host, int64) and
    edgel_offsets_device (int32) are every triplet's first row in both."""

    def __init__(self, batch: TripletBatch, device):
        import torch

        from .tracker import _require_gpu
        dev = _require_gpu(device)
        self.host = batch
        self.device = dev
        self.num_groups, self.num_samples = batch.num_groups, batch.num_samples
        self.target = torch.from_numpy(batch.target).to(dev)
        self.diff = torch.from_numpy(batch.diff).to(dev)
        self.edgels = torch.from_numpy(np.ascontiguousarray(np.concatenate(batch.locations))).to(dev)
        self.K = torch.from_numpy(np.ascontiguousarray(np.stack(batch.Ks))).to(dev)
        self.sample_group = torch.from_numpy(batch.sample_group).to(dev)
        self.sample_ordinal = torch.from_numpy(batch.sample_ordinal).to(dev)
        self.edgel_offsets = np.concatenate([[0], np.cumsum(batch.edgel_counts[:-1], dtype=np.int64)]).astype(np.int64)
        if int(batch.edgel_counts.astype(np.int64).sum()) > 0x7FFFFFFF:
            raise _abi.HCError("DeviceTripletBatch: more than 2^31 - 1 edgels in all")
        self.tangents = torch.from_numpy(np.ascontiguousarray(np.concatenate(batch.tangents))).to(dev)
        self.edgel_offsets_device = torch.from_numpy(self.edgel_offsets.astype(np.int32)).to(dev)
        g = np.zeros(batch.num_groups, GROUP_DTYPE)
        g["locations"] = self.edgels.data_ptr() + self.edgel_offsets * 24     # E x 6 floats per triplet
        g["K"] = self.K.data_ptr() + np.arange(batch.num_groups, dtype=np.int64) * 36
        g["num_edgels"] = batch.edgel_counts
        self.groups = torch.from_numpy(g.view(np.uint8).reshape(-1).copy()).to(dev)

    def group_edgels(self, t: int):
        """Triplet t's scoring set as a device tensor (a view of `edgels`)."""
        o = int(self.edgel_offsets[t])
        return self.edgels[o:o + int(self.host.edgel_counts[t])]

    def check(self) -> None:
        check_groups(self.host.sample_group, self.num_groups, self.num_samples, self.host.edgel_counts)
