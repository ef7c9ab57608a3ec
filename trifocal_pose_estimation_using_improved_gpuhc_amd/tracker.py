"""Device-side driver of the HIP tracker (one GPU / one process).

torch is used only as plumbing: device allocations, the HIP stream and events.
All compute runs in the native kernels behind include/hc_trifocal.h.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi
from .problem import Problem, RansacData

PATH_STATS_DTYPE = np.dtype([("steps", "<i4"), ("corrections", "<i4"), ("inliers21", "<i4"), ("inliers31", "<i4")])


# (abort, truncate, explicit_rk) -> the entry point (TrackMode of csrc/hc_kernels.hip)
_TRACK_ENTRY = {(True, True, False): "hc_trifocal_2op1p_30x30_track_abort",
                (False, True, False): "hc_trifocal_2op1p_30x30_track",
                (False, False, False): "hc_trifocal_2op1p_30x30_track_ph_codeopt",
                (False, False, True): "hc_trifocal_2op1p_30x30_track_ph"}


def _require_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _abi.HCError("the GPU-HC tracker needs a ROCm GPU (no CPU fallback exists)")
    return dev


@dataclass
class TrackResult:
    tracks: torch.Tensor          # (312N, 31, 2) float32 on device
    converge: torch.Tensor        # (312N,) uint8
    infinity: torch.Tensor        # (312N,) uint8
    stats: torch.Tensor | None    # (312N, 4) int32 [steps, corrections, inliers21, inliers31]
    found: torch.Tensor | None = None         # abort mode: (1,) uint8
    batch_index: torch.Tensor | None = None   # abort mode: (312N,) int32
    # grouped abort mode: found is the (T,) int32 per-triplet flag, found_ticks the (T,) int64
    # device clock of each triplet's first find (0: none)
    found_ticks: torch.Tensor | None = None
    # gated abort mode: (312N,) int32, the joint inlier count of every scored path, -1 elsewhere
    joint_inliers: torch.Tensor | None = None
    # adaptive sample limit: (T,) int32, in/out: each triplet's limit (its budget on entry of a fresh run)
    limit: torch.Tensor | None = None

    def host(self):
        out = dict(tracks=self.tracks.cpu().numpy(), converge=self.converge.cpu().numpy(),
                   infinity=self.infinity.cpu().numpy())
        if self.stats is not None:
            out["stats"] = self.stats.cpu().numpy().view(PATH_STATS_DTYPE).reshape(-1)
        if self.found_ticks is not None:
            out["found"] = self.found.cpu().numpy()
            out["found_ticks"] = self.found_ticks.cpu().numpy()
            out["batch_index"] = self.batch_index.cpu().numpy()
        elif self.found is not None:
            out["found"] = bool(self.found.cpu().item())
            out["batch_index"] = self.batch_index.cpu().numpy()
        if self.joint_inliers is not None:
            out["joint_inliers"] = self.joint_inliers.cpu().numpy()
        if self.limit is not None:
            out["limit"] = self.limit.cpu().numpy()
        return out


def gate_ratio(gate) -> float:
    """The min_joint_ratio of a gated launch from the caller's `gate`: a float
    (Python or numpy), finite and positive; anything else raises HCError."""
    if not isinstance(gate, (float, np.floating)):
        raise _abi.HCError(f"gate must be a float ratio, not {type(gate).__name__}")
    v = float(np.float32(gate))
    if not (np.isfinite(v) and v > 0.0):
        raise _abi.HCError(f"gate must be finite and positive as a float32 (got {gate!r})")
    return v


def need_table(num_edgels: int, confidence: float, min_samples: int = 1, max_samples: int = 2**31 - 1) -> np.ndarray:
    """hc_ransac_need_table: the (E + 1,) int32 table of the standard RANSAC
    rule for three edgels per sample; entry c is the number of samples needed
    for `confidence` after a hypothesis with c of E joint inliers,
    ceil(log(1 - p) / log(1 - (c / E)^3)) clamped to [min_samples, max_samples]."""
    E = int(num_edgels)
    need = np.empty(max(E, 0) + 1, np.int32)
    _abi.call("hc_ransac_need_table", E, float(confidence), int(min_samples), int(max_samples), _abi.ptr(need))
    return need


class AdaptiveStop:
    """The adaptive sample limit of a gated launch (launch_grouped(adaptive=...)):
    every scored path lowers its triplet's limit to the rule's sample count for
    its joint inlier count, and samples from the limit on are not tracked.

    confidence in (0, 1); min_samples >= 1; max_samples (default: the triplet's
    own sample count) caps a table's entries.  tables (optional): one int32
    array of E_t + 1 entries per triplet that replaces the built tables (another
    rule, or a test's)."""

    def __init__(self, confidence: float = 0.99, min_samples: int = 1, max_samples: int | None = None, tables=None):
        if isinstance(confidence, bool) or not isinstance(confidence, (float, np.floating)) or \
                not 0.0 < float(confidence) < 1.0:
            raise _abi.HCError(f"AdaptiveStop: confidence must be a float in (0, 1) (got {confidence!r})")
        for what, v in (("min_samples", min_samples), ("max_samples", max_samples)):
            if v is None and what == "max_samples":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise _abi.HCError(f"AdaptiveStop: {what} must be an integer >= 1 (got {v!r})")
        if max_samples is not None and int(max_samples) < int(min_samples):
            raise _abi.HCError("AdaptiveStop: max_samples < min_samples")
        if tables is not None:
            if isinstance(tables, np.ndarray) or not hasattr(tables, "__len__") or len(tables) < 1:
                raise _abi.HCError("AdaptiveStop: tables is a list of one array per triplet")
            tabs = []
            for t, tab in enumerate(tables):
                a = np.asarray(tab)
                if a.ndim != 1 or a.shape[0] < 2 or not np.issubdtype(a.dtype, np.integer) or \
                        (a < 0).any() or (a > 2**31 - 1).any():
                    raise _abi.HCError(f"AdaptiveStop: table {t} must hold E + 1 >= 2 non-negative int32 values")
                tabs.append(np.ascontiguousarray(a, np.int32))
            tables = tabs
        self.confidence, self.min_samples = float(confidence), int(min_samples)
        self.max_samples = None if max_samples is None else int(max_samples)
        self.tables = tables
        self._prepared = None   # (batch, need, need_offset): the device copies made for the last batch

    def host_tables(self, edgel_counts, sample_counts) -> list:
        """The triplets' tables: the caller's, checked against the edgel
        counts, or hc_ransac_need_table's."""
        if self.tables is not None:
            if len(self.tables) != len(edgel_counts) or \
                    any(t.shape[0] != int(e) + 1 for t, e in zip(self.tables, edgel_counts)):
                raise _abi.HCError("AdaptiveStop: one table of E + 1 entries per triplet")
            return self.tables
        return [need_table(int(e), self.confidence, self.min_samples,
                           max(self.max_samples if self.max_samples is not None else int(n), self.min_samples))
                for e, n in zip(edgel_counts, sample_counts)]

    def prepare(self, batch):
        """(need, need_offset), the device copies of the tables for batch (a
        multi.DeviceTripletBatch), made once per batch: call it before a launch
        that is recorded in a graph."""
        if self._prepared is None or self._prepared[0] is not batch:
            tabs = self.host_tables(batch.host.edgel_counts, [len(i) for i in batch.host.index])
            off = np.concatenate([[0], np.cumsum([t.shape[0] for t in tabs[:-1]], dtype=np.int64)]).astype(np.int64)
            self._prepared = (batch, torch.from_numpy(np.concatenate(tabs)).to(batch.device),
                              torch.from_numpy(off).to(batch.device))
        return self._prepared[1], self._prepared[2]


class DeviceTracker:
    """Holds the problem constants on one device and launches tracking runs.

    Mirrors what GPU_HC_Solver keeps per GPU (magmaHC/GPU_HC_Solver.cpp:137-184):
    start solutions, start parameters, the unified dH/dx||dH/dt index table.
    """

    def __init__(self, problem: Problem, device="cuda:0", max_steps=None, max_corrections=None,
                 delta_t_inc_steps=None):
        self.device = _require_gpu(device)
        self.L = _abi.lib()
        s = problem.settings
        self.settings = _abi.hcTrackSettings(
            int(max_steps if max_steps is not None else s.get("GPUHC_Max_Steps", 80)),
            int(max_corrections if max_corrections is not None else s.get("GPUHC_Max_Correction_Steps", 3)),
            int(delta_t_inc_steps if delta_t_inc_steps is not None else
                s.get("GPUHC_Num_Of_Steps_to_Increase_Delta_t", 4)))
        dev = self.device
        self.start_sols = torch.from_numpy(problem.start_sols).to(dev)
        self.start_params = torch.from_numpy(problem.start_params).to(dev)
        self.unified = torch.from_numpy(problem.unified_index).to(dev)
        self.ws_bytes = int(self.L.hc_trifocal_workspace_size())
        self.workspace = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.edgels = None
        self.K = None
        self._problem = problem       # track_p2c: the PH tables and the start parameters on the host
        self._p2c_default = None      # track_p2c: (device tables, map) of p2c.tables_from_ph, made on first use

    def set_ransac_data(self, data: RansacData):
        self.edgels = torch.from_numpy(np.ascontiguousarray(data.locations)).to(self.device)
        self.K = torch.from_numpy(np.ascontiguousarray(data.K)).to(self.device)

    def allocate(self, num_samples: int, stats: bool = True, abort: bool = False) -> TrackResult:
        n = num_samples * 312
        dev = self.device
        r = TrackResult(
            tracks=torch.empty((n, 31, 2), dtype=torch.float32, device=dev),
            converge=torch.empty(n, dtype=torch.uint8, device=dev),
            infinity=torch.empty(n, dtype=torch.uint8, device=dev),
            stats=torch.empty((n, 4), dtype=torch.int32, device=dev) if stats else None)
        if abort:
            r.found = torch.zeros(1, dtype=torch.uint8, device=dev)
            r.batch_index = torch.full((n,), -1, dtype=torch.int32, device=dev)
        return r

    def reset_tracks(self, r: TrackResult):
        """Feed_Start_Sols_for_Intermediate_Homotopy: every sample starts at the start solutions."""
        n = r.tracks.shape[0] // 312
        r.tracks.view(n, 312, 31, 2).copy_(self.start_sols.unsqueeze(0).expand(n, -1, -1, -1))
        if r.found is not None:
            r.found.zero_()
            r.batch_index.fill_(-1)
        if r.found_ticks is not None:
            r.found_ticks.zero_()
        if r.joint_inliers is not None:
            r.joint_inliers.fill_(-1)

    def _workspace(self, workspace: torch.Tensor | None) -> torch.Tensor:
        """A launch's workspace (default: the tracker's own), at least the minimum size."""
        ws_t = workspace if workspace is not None else self.workspace
        if ws_t.numel() < self.ws_bytes:
            raise _abi.HCError("workspace too small")
        return ws_t

    def _track_args(self, r: TrackResult, target: torch.Tensor, diff: torch.Tensor, sample_offset: int,
                    num_samples: int) -> _abi.hcTrackArgs:
        """hcTrackArgs of samples [sample_offset, sample_offset + num_samples) of
        target / diff, tracked into the matching rows of r."""
        p0 = sample_offset * 312
        a = _abi.hcTrackArgs()
        a.sub_ransac_iters = num_samples
        a.settings = self.settings
        a.start_sols = self.start_sols.data_ptr()
        a.start_sols_array = None
        a.tracks = r.tracks[p0:].data_ptr()
        a.track_array = None
        a.start_params = self.start_params.data_ptr()
        a.target_params = target[sample_offset:].data_ptr()
        a.diff_params = diff[sample_offset:].data_ptr()
        a.unified_index = self.unified.data_ptr()
        a.converge = r.converge[p0:].data_ptr()
        a.infinity = r.infinity[p0:].data_ptr()
        a.stats = r.stats[p0:].data_ptr() if r.stats is not None else None
        return a

    def allocate_grouped(self, batch, stats: bool = True, gate: bool = False, adaptive: bool = False) -> TrackResult:
        """Buffers of a grouped launch over batch (a multi.DeviceTripletBatch):
        as allocate(abort=True), with one found word and one tick per triplet;
        gate: also the per-path joint inlier counts of a gated launch;
        adaptive: those and the triplets' sample limits, set to each triplet's
        sample count (the budget of a fresh run)."""
        gate = gate or adaptive
        r = self.allocate(batch.num_samples, stats=stats, abort=True)
        r.found = torch.zeros(batch.num_groups, dtype=torch.int32, device=self.device)
        r.found_ticks = torch.zeros(batch.num_groups, dtype=torch.int64, device=self.device)
        if gate:
            r.joint_inliers = torch.full((batch.num_samples * 312,), -1, dtype=torch.int32, device=self.device)
        if adaptive:
            r.limit = torch.from_numpy(np.array([len(i) for i in batch.host.index], np.int32)).to(self.device)
        return r

    def launch_grouped(self, batch, r: TrackResult, stream: torch.cuda.Stream | None = None,
                       workspace: torch.Tensor | None = None, inflight_stop: bool = False, gate=None,
                       adaptive=None) -> None:
        """Enqueue one grouped (multi-triplet) abort-mode run on `stream` (no
        synchronisation): hc_trifocal_2op1p_30x30_track_abort_grouped over all of
        batch's samples (a multi.DeviceTripletBatch) into r (allocate_grouped).
        A path is skipped once the flag of its own triplet is set -- also when
        the caller set it: r.found is in/out, the carry-over between launches --
        and scored on its own triplet's edgels; r.found_ticks[t] receives the
        device clock of triplet t's first find (read_timestamps gives the
        launch's start).  inflight_stop as in launch().
        gate (a float ratio, default None: the launch above, unchanged): the
        stop rule is the joint inlier support instead
        (hc_trifocal_2op1p_30x30_track_abort_gated): a converged path that
        passes the pose-support candidate filter is scored on its own triplet's
        E edgels with the pose-support test, and sets its triplet's flag iff its
        joint count (edgels within 2 px in both views) is at least gate * E.
        r.joint_inliers (allocate_grouped(gate=True)) receives every scored
        path's joint count, r.stats its two per-view counts.
        adaptive (an AdaptiveStop, default None): the gated launch's adaptive
        mode (include/adaptive/hc_trifocal_adaptive.h); without gate the ratio
        is 2.0, which never fires.  A path is also skipped once its sample's
        index within its triplet (batch.sample_ordinal) has reached r.limit[t]
        (allocate_grouped(adaptive=True); in/out, the carry-over between
        launches as r.found is), and a scored path lowers r.limit[t] to its
        triplet's table entry of its joint count."""
        ratio = None if gate is None else gate_ratio(gate)
        if adaptive is not None:
            if not isinstance(adaptive, AdaptiveStop):
                raise _abi.HCError(f"adaptive must be an AdaptiveStop, not {type(adaptive).__name__}")
            if ratio is None:
                ratio = 2.0
        if batch.target.device != self.start_sols.device:
            raise _abi.HCError("the batch lives on another device")
        batch.check()   # group ids and edgel counts: the kernels do not validate them
        n, T = batch.num_samples, batch.num_groups
        if n * 312 > r.tracks.shape[0] or r.found is None or r.found_ticks is None or r.found.numel() < T or \
                r.found_ticks.numel() < T or r.found.dtype != torch.int32 or r.found_ticks.dtype != torch.int64:
            raise _abi.HCError("result buffers do not fit the batch (allocate_grouped)")
        if ratio is not None and (r.joint_inliers is None or r.joint_inliers.numel() < n * 312 or
                                  r.joint_inliers.dtype != torch.int32):
            raise _abi.HCError("a gated launch needs r.joint_inliers (allocate_grouped(gate=True))")
        if adaptive is not None and (r.limit is None or r.limit.numel() < T or r.limit.dtype != torch.int32):
            raise _abi.HCError("an adaptive launch needs r.limit (allocate_grouped(adaptive=True))")
        ws_t = self._workspace(workspace)
        a = self._track_args(r, batch.target, batch.diff, 0, n)
        g = _abi.hcGroupedAbortArgs()
        g.num_groups = T
        g.groups = batch.groups.data_ptr()
        g.sample_group = batch.sample_group.data_ptr()
        g.group_found = r.found.data_ptr()
        g.trifocal_sols_batch_index = r.batch_index.data_ptr()
        g.group_found_ticks = r.found_ticks.data_ptr()
        g.inflight_stop = 1 if inflight_stop else 0
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        name, blocks = "hc_trifocal_2op1p_30x30_track_abort_grouped", [C.byref(a), C.byref(g)]
        if ratio is not None:
            ag = _abi.hcAdaptiveGate()   # its head alone is the plain gated launch's hcJointGate
            ag.head.min_joint_ratio = ratio
            ag.head.joint_inliers = r.joint_inliers.data_ptr()
            if adaptive is not None:
                need, need_offset = adaptive.prepare(batch)
                ag.head.pad = _abi.HC_GATE_ADAPTIVE
                ag.need, ag.need_offset = need.data_ptr(), need_offset.data_ptr()
                ag.sample_ordinal = batch.sample_ordinal.data_ptr()
                ag.group_limit = r.limit.data_ptr()
            name = "hc_trifocal_2op1p_30x30_track_abort_gated"
            blocks.append(C.cast(C.pointer(ag), C.POINTER(_abi.hcJointGate)))
        _abi.call(name, *blocks, _abi.ptr(ws_t), self.ws_bytes, _abi.ptr(s))

    def track_grouped(self, batch, inflight_stop: bool = False, stats: bool = True, found=None,
                      gate=None, adaptive=None, limit=None) -> TrackResult:
        """Synchronous convenience wrapper of launch_grouped, as track(abort=True):
        batch is a multi.TripletBatch or its device copy.  found (optional, T
        values): the triplets' flags on entry (a set one skips its triplet).
        gate (a float ratio): the gated launch; the result carries joint_inliers.
        adaptive (an AdaptiveStop): the adaptive sample limit; the result
        carries limit, the triplets' final limits.  limit (optional, T values):
        the limits on entry (default: each triplet's sample count)."""
        if gate is not None:
            gate_ratio(gate)
        if adaptive is not None and not isinstance(adaptive, AdaptiveStop):
            raise _abi.HCError(f"adaptive must be an AdaptiveStop, not {type(adaptive).__name__}")
        if limit is not None and adaptive is None:
            raise _abi.HCError("limit is the adaptive launch's (pass adaptive=AdaptiveStop(...))")
        if not hasattr(batch, "groups"):
            batch = batch.to(self.device)
        r = self.allocate_grouped(batch, stats=stats, gate=gate is not None, adaptive=adaptive is not None)
        self.reset_tracks(r)
        if found is not None:
            f = np.ascontiguousarray(found, np.int32).reshape(-1)
            if f.shape[0] != batch.num_groups:
                raise _abi.HCError("one initial flag per triplet")
            r.found.copy_(torch.from_numpy(f))
        if limit is not None:
            lim = np.ascontiguousarray(limit, np.int64).reshape(-1)
            if lim.shape[0] != batch.num_groups or (lim < 0).any() or (lim > 2**31 - 1).any():
                raise _abi.HCError("one initial limit per triplet, each in [0, 2^31)")
            r.limit.copy_(torch.from_numpy(lim.astype(np.int32)))
        self.launch_grouped(batch, r, inflight_stop=inflight_stop, gate=gate, adaptive=adaptive)
        torch.cuda.synchronize(self.device)
        self.workspace_status()
        return r

    def launch(self, target: torch.Tensor, diff: torch.Tensor, r: TrackResult, abort: bool = False,
               stream: torch.cuda.Stream | None = None, workspace: torch.Tensor | None = None,
               sample_offset: int = 0, num_samples: int | None = None, inflight_stop: bool = False,
               truncate: bool = True, explicit_rk: bool = False, time_slicing: bool = True,
               peer_found=None) -> None:
        """Enqueue one tracking run on `stream` (no synchronisation).

        Samples [sample_offset, sample_offset + num_samples) of `target`/`diff`
        are tracked into the matching rows of `r` (defaults: all of them); the
        launch's batch ids (abort-mode batch_index values) are local to it.
        inflight_stop (abort mode): paths in flight also stop once a pose is
        found (hcAbortArgs::inflight_stop; default: the reference's semantics,
        they run to completion).  truncate=False: no depth-sign path
        truncation (the archived ..._PH_CodeOpt kernel, hc_trifocal_2op1p_30x30_track_ph_codeopt);
        with explicit_rk=True as well, the archived ..._PH kernel (hc_trifocal_2op1p_30x30_track_ph).
        peer_found (abort mode): a sharding.SharedFlag of a multi-GPU run
        (hcAbortArgs::peer_found): set here on a find, polled before each path.
        time_slicing (tracking launches): suspend and resume paths at step
        boundaries so every path starts early (hc_trifocal_workspace_size_for;
        bit-identical results).  The default workspace grows to the size that
        enables it; a caller's workspace enables it if it is large enough.
        Growing the default workspace synchronises the device, so a launch that
        is recorded in a graph (torch.cuda.graph) must pass its own workspace,
        already sized: new_workspace(num_samples), or new_workspace() to run
        without slicing (tests/test_gpu_graph_replay.py)."""
        if num_samples is None:
            num_samples = target.shape[0] - sample_offset
        if num_samples < 0 or sample_offset < 0 or sample_offset + num_samples > target.shape[0] or \
                (sample_offset + num_samples) * 312 > r.tracks.shape[0]:
            raise _abi.HCError("sample range outside the buffers")
        if workspace is None and not abort and time_slicing:
            need = int(self.L.hc_trifocal_workspace_size_for_steps(num_samples, self.settings.max_steps))
            if self.workspace.numel() < need:
                # grown rarely (the first sliced launch of a size): the old
                # workspace may still be in use by a launch on any stream, and
                # the new one is zero-filled on the current stream, which need
                # not be `stream` -- synchronise on both sides of the swap
                torch.cuda.synchronize(self.device)
                self.workspace = torch.zeros(need, dtype=torch.uint8, device=self.device)
                torch.cuda.synchronize(self.device)
        ws_t = self._workspace(workspace)
        wsb = ws_t.numel() if (time_slicing and not abort) else self.ws_bytes
        a = self._track_args(r, target, diff, sample_offset, num_samples)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if abort and not truncate:
            raise _abi.HCError("abort mode always truncates paths (..._TrunRANSAC.cu)")
        if explicit_rk and truncate:
            raise _abi.HCError("the archived ..._PH kernel has no path truncation: pass truncate=False")
        blocks = [C.byref(a)]   # hcTrackArgs, then the mode's own argument block
        if abort:
            if self.edgels is None:
                raise _abi.HCError("abort mode needs set_ransac_data() first")
            ab = _abi.hcAbortArgs()
            ab.num_triplet_edgels = self.edgels.shape[0]
            ab.triplet_edge_locations = self.edgels.data_ptr()
            ab.intrinsic_matrix = self.K.data_ptr()
            ab.found_trifocal_sols = r.found.data_ptr()
            ab.trifocal_sols_batch_index = r.batch_index[sample_offset * 312:].data_ptr()
            ab.inflight_stop = 1 if inflight_stop else 0
            ab.peer_found = None if peer_found is None else peer_found.ptr
            blocks.append(C.byref(ab))
        _abi.call(_TRACK_ENTRY[bool(abort), bool(truncate), bool(explicit_rk)], *blocks, _abi.ptr(ws_t), wsb,
                  _abi.ptr(s))

    def new_workspace(self, num_samples: int = 0) -> torch.Tensor:
        """A workspace; with num_samples > 0, large enough for time slicing of
        tracking launches of up to that many samples."""
        n = (int(self.L.hc_trifocal_workspace_size_for_steps(num_samples, self.settings.max_steps))
             if num_samples > 0 else self.ws_bytes)
        return torch.zeros(n, dtype=torch.uint8, device=self.device)

    def launch_abort_chunked(self, target: torch.Tensor, diff: torch.Tensor, r: TrackResult, chunk_samples: int,
                             workspaces: list, group=None, stream: torch.cuda.Stream | None = None,
                             inflight_stop: bool = False, peer_found=None, max_count: int | None = None) -> list:
        """Abort-mode run of all of target's samples in chunks, with the
        cross-rank early-stop flag (sharding.run_abort_chunks): the launches
        and the flag reductions share one stream.  workspaces: one per chunk
        (grown as needed).  peer_found: a sharding.SharedFlag, so the launches
        also stop on another rank's find within a path (not only at the next
        chunk boundary).  max_count: the largest shard over the ranks
        (sharding.max_shard), so the chunk count needs no host-side agreement.
        Returns the (offset, count) chunks."""
        from . import sharding
        parts = sharding.chunks(target.shape[0], chunk_samples)
        while len(workspaces) < len(parts):
            workspaces.append(self.new_workspace())
        s = stream if stream is not None else torch.cuda.current_stream(self.device)

        def one(k, off, n):
            self.launch(target, diff, r, abort=True, stream=s, workspace=workspaces[k], sample_offset=off,
                        num_samples=n, inflight_stop=inflight_stop, peer_found=peer_found)
        sharding.run_abort_chunks(one, r.found, target.shape[0], chunk_samples, group=group, stream=s,
                                  max_count=max_count)
        return parts

    def workspace_status(self, workspace: torch.Tensor | None = None) -> None:
        """Raises HCError if the last launch on workspace failed on the device:
        HC_ERROR_TABLE (the index table does not fit the compaction; outputs
        untouched) or HC_ERROR_DEVICE (time slicing: a suspended path's ring
        entry never came or the ring overflowed; the lost path's outputs are
        not written; diagnostics in the control block's ring_fail words)."""
        ws = workspace if workspace is not None else self.workspace
        _abi.call("hc_trifocal_workspace_status", _abi.ptr(ws))

    def read_timestamps(self, workspace: torch.Tensor | None = None):
        """(start_ticks, found_ticks, tick_hz) of the last launch on workspace."""
        a, b, hz = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        ws = workspace if workspace is not None else self.workspace
        _abi.call("hc_trifocal_read_timestamps", _abi.ptr(ws), C.byref(a), C.byref(b), C.byref(hz))
        return a.value, b.value, hz.value

    def track(self, target: np.ndarray, diff: np.ndarray, abort: bool = False, stats: bool = True,
              inflight_stop: bool = False, truncate: bool = True, explicit_rk: bool = False,
              time_slicing: bool = True) -> TrackResult:
        """Synchronous convenience wrapper: H2D params, reset tracks, launch, sync, status check."""
        tgt = torch.from_numpy(np.ascontiguousarray(target, np.float32)).to(self.device)
        dif = torch.from_numpy(np.ascontiguousarray(diff, np.float32)).to(self.device)
        r = self.allocate(tgt.shape[0], stats=stats, abort=abort)
        self.reset_tracks(r)
        self.launch(tgt, dif, r, abort=abort, inflight_stop=inflight_stop, truncate=truncate, explicit_rk=explicit_rk,
                    time_slicing=time_slicing)
        torch.cuda.synchronize(self.device)
        self.workspace_status()
        return r

    def launch_p2c(self, tables, coeffs_hx: torch.Tensor, coeffs_ht: torch.Tensor, r: TrackResult,
                   stream: torch.cuda.Stream | None = None, workspace: torch.Tensor | None = None,
                   num_samples: int | None = None) -> None:
        """Enqueue one run of the archived P2C tracker on `stream` (no
        synchronisation): hc_trifocal_2op1p_30x30_track_p2c over the first
        num_samples samples (default: all) of the coefficient blocks coeffs_hx
        (N, 38, 3, 2) and coeffs_ht (N, 38, 2, 2) into r.  tables: the device
        tensors (hx_index, ht_index) of the P2C index tables (p2c_tables)."""
        hx, ht = tables
        if num_samples is None:
            num_samples = coeffs_hx.shape[0]
        if num_samples < 0 or num_samples > coeffs_hx.shape[0] or num_samples > coeffs_ht.shape[0] or \
                num_samples * 312 > r.tracks.shape[0]:
            raise _abi.HCError("sample range outside the buffers")
        if hx.numel() != 28800 or ht.numel() != 2400 or hx.dtype != torch.int32 or ht.dtype != torch.int32:
            raise _abi.HCError("P2C tables: 28800 and 2400 int32 values")
        if tuple(coeffs_hx.shape[1:]) != (38, 3, 2) or tuple(coeffs_ht.shape[1:]) != (38, 2, 2) or \
                coeffs_hx.dtype != torch.float32 or coeffs_ht.dtype != torch.float32 or \
                not coeffs_hx.is_contiguous() or not coeffs_ht.is_contiguous():
            raise _abi.HCError("P2C coefficient blocks: contiguous float32 (N, 38, 3, 2) and (N, 38, 2, 2)")
        ws_t = self._workspace(workspace)
        a = _abi.hcTrackArgs()
        a.sub_ransac_iters = num_samples
        a.settings = self.settings
        a.start_sols = self.start_sols.data_ptr()
        a.tracks = r.tracks.data_ptr()
        a.converge = r.converge.data_ptr()
        a.infinity = r.infinity.data_ptr()
        a.stats = r.stats.data_ptr() if r.stats is not None else None
        pa = _abi.hcP2cArgs(hx.data_ptr(), ht.data_ptr(), coeffs_hx.data_ptr(), coeffs_ht.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _abi.call("hc_trifocal_2op1p_30x30_track_p2c", C.byref(a), C.byref(pa), _abi.ptr(ws_t), self.ws_bytes,
                  _abi.ptr(s))

    def p2c_tables(self, tables):
        """(hx_index, ht_index) host arrays -> the device tensors launch_p2c takes."""
        hx, ht = tables
        return (torch.from_numpy(np.ascontiguousarray(hx, np.int32).reshape(-1)).to(self.device),
                torch.from_numpy(np.ascontiguousarray(ht, np.int32).reshape(-1)).to(self.device))

    def track_p2c(self, target: np.ndarray, diff: np.ndarray, tables=None, coeff_map=None,
                  stats: bool = True) -> TrackResult:
        """Synchronous convenience wrapper of the archived P2C tracker: the
        samples' coefficient blocks from diff (p2c.coefficients, on the host),
        H2D, reset tracks, launch_p2c, sync, status check.  tables: the P2C
        index tables (hx_index, ht_index) with their coeff_map (38, 2)
        (p2c.derive_coeff_map); by default those p2c.tables_from_ph makes of the
        problem's PH tables.  target is not read (diff = target - start)."""
        from . import p2c
        if tables is None:
            if self._p2c_default is None:
                hx, ht, m = p2c.tables_from_ph(self._problem)
                self._p2c_default = (self.p2c_tables((hx, ht)), m)
            dev_tables, default_map = self._p2c_default
            if coeff_map is None:
                coeff_map = default_map
        else:
            if coeff_map is None:
                coeff_map = p2c.derive_coeff_map(self._problem, tables[0], tables[1])
            dev_tables = self.p2c_tables(tables)
        chx, cht = p2c.coefficients(coeff_map, self._problem.start_params, diff)
        chx_t, cht_t = torch.from_numpy(chx).to(self.device), torch.from_numpy(cht).to(self.device)
        r = self.allocate(chx.shape[0], stats=stats)
        self.reset_tracks(r)
        self.launch_p2c(dev_tables, chx_t, cht_t, r)
        torch.cuda.synchronize(self.device)
        self.workspace_status()
        return r

    def first_found_seconds(self) -> float:
        v = C.c_double(0.0)
        _abi.call("hc_trifocal_read_timings", _abi.ptr(self.workspace), C.byref(v))
        return v.value


def cgesv_batched(A: np.ndarray, b: np.ndarray, device="cuda:0") -> np.ndarray:
    """Batched tracker-LU solve of n 30x30 complex systems (A row-major (n,30,30,2))."""
    dev = _require_gpu(device)
    At = torch.from_numpy(np.ascontiguousarray(A, np.float32)).to(dev)
    bt = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev)
    xt = torch.empty_like(bt)
    n = At.shape[0]
    _abi.call("hc_cgesv_30x30_batched", n, _abi.ptr(At), _abi.ptr(bt), _abi.ptr(xt),
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    return xt.cpu().numpy()


def cgesv_struct_batched(A: np.ndarray, b: np.ndarray, device="cuda:0") -> np.ndarray:
    """The throughput tracker's structure-specialised solve of n 30x30 complex
    systems (layout of cgesv_batched).  Raises HCError (HC_ERROR_INVALID_VALUE)
    when an entry outside the compiled-in structure is non-zero."""
    dev = _require_gpu(device)
    At = torch.from_numpy(np.ascontiguousarray(A, np.float32)).to(dev)
    bt = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev)
    xt = torch.empty_like(bt)
    _abi.call("hc_cgesv_30x30_struct_batched", At.shape[0], _abi.ptr(At), _abi.ptr(bt), _abi.ptr(xt),
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    return xt.cpu().numpy()


def cgesv_variant_batched(variant, A: np.ndarray, b: np.ndarray, device="cuda:0") -> np.ndarray:
    """One of the tracker's sparse solves alone (hcLuVariant: its number, or its
    name in _abi.LU_VARIANTS) on n 30x30 complex systems (layout of
    cgesv_batched).  Raises HCError (HC_ERROR_INVALID_VALUE) for an unknown
    variant and, in the variants with the compiled-in structure, when an entry
    outside it is non-zero."""
    dev = _require_gpu(device)
    if isinstance(variant, str):
        variant = _abi.LU_VARIANTS.index(variant)
    At = torch.from_numpy(np.ascontiguousarray(A, np.float32)).to(dev)
    bt = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev)
    xt = torch.empty_like(bt)
    _abi.call("hc_cgesv_30x30_variant_batched", int(variant), At.shape[0], _abi.ptr(At), _abi.ptr(bt), _abi.ptr(xt),
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    return xt.cpu().numpy()


def eval_batched(unified: np.ndarray, x: np.ndarray, p: np.ndarray, d: np.ndarray, device="cuda:0"):
    """Batched dH/dx, dH/dt, H at (x, p) with the tracker's compacted tables."""
    dev = _require_gpu(device)
    n = x.shape[0]
    U = torch.from_numpy(np.ascontiguousarray(unified, np.int32)).to(dev)
    X = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    P = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    D = torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(dev)
    HX = torch.empty((n, 30, 30, 2), dtype=torch.float32, device=dev)
    HT = torch.empty((n, 30, 2), dtype=torch.float32, device=dev)
    H = torch.empty((n, 30, 2), dtype=torch.float32, device=dev)
    wsb = int(_abi.lib().hc_trifocal_workspace_size())
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    _abi.call("hc_trifocal_eval_batched", n, *(_abi.ptr(t) for t in (U, X, P, D, HX, HT, H, ws)), wsb,
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    return HX.cpu().numpy(), HT.cpu().numpy(), H.cpu().numpy()


def eval_variant_batched(variant, unified: np.ndarray, x: np.ndarray, target: np.ndarray, diff: np.ndarray,
                         start_params: np.ndarray, t: np.ndarray, kind: np.ndarray, redo: bool = False,
                         device="cuda:0", workspace: torch.Tensor | None = None):
    """hc_trifocal_eval_variant_batched (include/eval/hc_eval_testing.h): one
    stage's evaluations as a tracking kernel runs them, at n points; point i in
    path slot i % 8, points 2k and 2k + 1 in one wave.  variant: hcEvalVariant,
    its number or its name in _abi.EVAL_VARIANTS.  x (n, 31, 2), target and diff
    (n, 34, 2), t (n,), kind (n,) uint8 (0: the negated dH/dt, 1: H).  Returns
    (Hx (n, 30, 30, 2), rhs (n, 30, 2), ent_ok (n, 32) uint8: the lanes' verdicts,
    all 255 for the packed variant, which leaves them untouched).  workspace: a
    device tensor to run in (default: a fresh one)."""
    dev = _require_gpu(device)
    if isinstance(variant, str):
        variant = _abi.EVAL_VARIANTS.index(variant)
    n = x.shape[0]
    U = torch.from_numpy(np.ascontiguousarray(unified, np.int32)).to(dev)
    X = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    TG = torch.from_numpy(np.ascontiguousarray(target, np.float32)).to(dev)
    DF = torch.from_numpy(np.ascontiguousarray(diff, np.float32)).to(dev)
    SP = torch.from_numpy(np.ascontiguousarray(start_params, np.float32)).to(dev)
    T = torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(dev)
    K = torch.from_numpy(np.ascontiguousarray(kind, np.uint8)).to(dev)
    if tuple(X.shape) != (n, 31, 2) or tuple(TG.shape) != (n, 34, 2) or tuple(DF.shape) != (n, 34, 2) or \
            tuple(SP.shape) != (34, 2) or tuple(T.shape) != (n,) or tuple(K.shape) != (n,) or U.numel() != 38880:
        raise _abi.HCError("eval_variant_batched: x (n, 31, 2), target and diff (n, 34, 2), start_params (34, 2), "
                           "t and kind (n,), a unified index of 38880 values")
    HX = torch.empty((n, 30, 30, 2), dtype=torch.float32, device=dev)
    RHS = torch.empty((n, 30, 2), dtype=torch.float32, device=dev)
    OK = torch.full((n, 32), 255, dtype=torch.uint8, device=dev)
    wsb = int(_abi.lib().hc_trifocal_workspace_size())
    ws = workspace if workspace is not None else torch.zeros(wsb, dtype=torch.uint8, device=dev)
    if ws.numel() * ws.element_size() < wsb:
        raise _abi.HCError("eval_variant_batched: workspace too small")
    _abi.call("hc_trifocal_eval_variant_batched", int(variant), _abi.HC_EVAL_REDO if redo else 0, n,
              *(_abi.ptr(v) for v in (U, X, TG, DF, SP, T, K, HX, RHS, OK, ws)), ws.numel() * ws.element_size(),
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    return HX.cpu().numpy(), RHS.cpu().numpy(), OK.cpu().numpy()


def compact_rows_batched(unified: np.ndarray, x: np.ndarray, target: np.ndarray, diff: np.ndarray,
                         start_params: np.ndarray, t: np.ndarray, kind: np.ndarray, device="cuda:0"):
    """hc_trifocal_compact_rows_batched (include/lu/hc_lu_compact_testing.h): the
    rows of dH/dx in the compact form the throughput tracker gathers for its fused
    solve, at n points; arguments as eval_variant_batched's.  Returns (rows (n, 30,
    16, 2): position p of row r is column hc_lu_compact_column(r, p), rhs (n, 30, 2))."""
    dev = _require_gpu(device)
    n = x.shape[0]
    U = torch.from_numpy(np.ascontiguousarray(unified, np.int32)).to(dev)
    X = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    TG = torch.from_numpy(np.ascontiguousarray(target, np.float32)).to(dev)
    DF = torch.from_numpy(np.ascontiguousarray(diff, np.float32)).to(dev)
    SP = torch.from_numpy(np.ascontiguousarray(start_params, np.float32)).to(dev)
    T = torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(dev)
    K = torch.from_numpy(np.ascontiguousarray(kind, np.uint8)).to(dev)
    if tuple(X.shape) != (n, 31, 2) or tuple(TG.shape) != (n, 34, 2) or tuple(DF.shape) != (n, 34, 2) or \
            tuple(SP.shape) != (34, 2) or tuple(T.shape) != (n,) or tuple(K.shape) != (n,) or U.numel() != 38880:
        raise _abi.HCError("compact_rows_batched: x (n, 31, 2), target and diff (n, 34, 2), start_params (34, 2), "
                           "t and kind (n,), a unified index of 38880 values")
    ROWS = torch.full((n, 30, _abi.LU_COMPACT_WIDTH, 2), float("nan"), dtype=torch.float32, device=dev)
    RHS = torch.empty((n, 30, 2), dtype=torch.float32, device=dev)
    OK = torch.full((n, 32), 255, dtype=torch.uint8, device=dev)
    wsb = int(_abi.lib().hc_trifocal_workspace_size())
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)   # the hook runs on the null stream
    _abi.call("hc_trifocal_compact_rows_batched", n, *(_abi.ptr(v) for v in (U, X, TG, DF, SP, T, K, ROWS, RHS, OK, ws)),
              wsb)
    torch.cuda.synchronize(dev)
    return ROWS.cpu().numpy(), RHS.cpu().numpy()
