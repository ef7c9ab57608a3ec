"""Pose recovery, maximal-support selection and GT pose error.

Device side: hc_trifocal_pose_support (include/hc_pose.h, csrc/hc_pose.hip)
replaces the host loops of Evaluations::Transform_GPUHC_Sols_to_Trifocal_Relative_Pose
(magmaHC/Evaluations.cpp:298-358) and get_Solution_with_Maximal_Support
(:382-504).  Host side: hc_pose_merge (per-GPU selections -> one) and
hc_pose_residuals (Measure_Relative_Pose_Error, :523-543).

Joint selection (not in the reference): hc_trifocal_pose_support_joint and its
grouped form select one hypothesis for both views, by the number of edgels that
are inliers in both; hc_trifocal_pose_inlier_mask lists those edgels and
hc_pose_merge_joint merges per-launch selections (pose_support_joint,
pose_support_joint_grouped, inlier_mask, merge_joint below).

Refinement (not in the reference): hc_trifocal_pose_refine and its grouped form
(include/refine/hc_pose_refine.h) fit a joint selection's pose to its joint
inliers on the device and return a selection of the same layout
(launch_refine_joint, refine_joint, refine_joint_grouped below).

Top-k (not in the reference): the calls of include/topk/hc_pose_topk.h rank the
k best joint candidates from the per-path counts, refine all k on one scene in
one launch and select the refined one with the most joint inliers (topk_joint,
refine_topk, their grouped forms, merge_topk, and select_refined, which chains
joint support, top-k and refine-and-select on one stream).

Relative scale (not in the reference): a mode of the four refine calls
(include/scale/hc_pose_scale.h) fits scale31, the length of t31 in units of
t21, by three-view transfer support after the refinement (fit_scale,
transfer_mask and select_by_transfer on the refine wrappers; fit_scale31 is the
scale-only form).

Three-view refinement (not in the reference): a further mode of the same calls
(include/threeview/hc_pose_threeview.h) refines both views and the scale
jointly on the three-view transfer after the refinement and the scale fit
(three_view and three_view_iterations on the refine wrappers; it implies
fit_scale).

Structure (not in the reference): a fourth stage of the same calls
(include/structure/hc_pose_structure.h) writes the 3D edgels, point and
tangent, that the pose that goes out explains in all three views (structure and
tangents on the refine wrappers; it implies three_view; reconstruct is the
structure-only form and write_edgels3d a text writer).

The four pose-support calls (per view / joint, one triplet / grouped) share one
launcher and one synchronous wrapper (_launch, _run), parameterised by a _Rule.
Every native call goes through the signature table of _abi: buffers and streams
are passed as _abi.ptr(x), hcStatus entry points are called by _abi.call(name, ...).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _abi
from .problem import RansacData

SEL_BYTES = _abi.POSE_SELECTION_BYTES
JOINT_SEL_BYTES = _abi.TRIFOCAL_SELECTION_BYTES


def _struct_from_raw(cls, nbytes, raw):
    b = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    return cls.from_buffer_copy(np.ascontiguousarray(b, np.uint8).tobytes()[:nbytes])


def selection_struct(raw: np.ndarray | torch.Tensor) -> _abi.hcPoseSelection:
    return _struct_from_raw(_abi.hcPoseSelection, SEL_BYTES, raw)


def selection_dict(s: _abi.hcPoseSelection) -> dict:
    return dict(num_candidates=s.num_candidates, path21=s.path21, inliers21=s.inliers21, path31=s.path31,
                inliers31=s.inliers31, key21=s.key21, key31=s.key31,
                R21=np.array(s.R21[:], np.float32), t21=np.array(s.t21[:], np.float32),
                R31=np.array(s.R31[:], np.float32), t31=np.array(s.t31[:], np.float32))


# One hypothesis for both views, scored on the edgels that are inliers in view
# 1-2 and in view 1-3 (hcTrifocalSelection, include/hc_pose.h).
def joint_selection_struct(raw) -> _abi.hcTrifocalSelection:
    if isinstance(raw, _abi.hcTrifocalSelection):
        return raw
    return _struct_from_raw(_abi.hcTrifocalSelection, JOINT_SEL_BYTES, raw)


def joint_selection_dict(s: _abi.hcTrifocalSelection) -> dict:
    return dict(num_candidates=s.num_candidates, path=s.path, inliers=s.inliers, inliers21=s.inliers21,
                inliers31=s.inliers31, key=s.key,
                R21=np.array(s.R21[:], np.float32), t21=np.array(s.t21[:], np.float32),
                R31=np.array(s.R31[:], np.float32), t31=np.array(s.t31[:], np.float32),
                scale31=np.float32(s.scale31))


def joint_selection_from_dict(d: dict) -> _abi.hcTrifocalSelection:
    s = _abi.hcTrifocalSelection()
    for k in ("num_candidates", "path", "inliers", "inliers21", "inliers31", "key"):
        setattr(s, k, int(d[k]))
    for k in ("R21", "t21", "R31", "t31"):
        getattr(s, k)[:] = [float(v) for v in d[k]]
    s.scale31 = float(d["scale31"])
    return s


# A selection rule: the entry point's name (+ "_grouped"), the int32 columns of
# its per-path counts, and its selection struct's size and converters.
_Rule = namedtuple("_Rule", "name columns sel_bytes struct to_dict")
_PER_VIEW = _Rule("pose_support", 2, SEL_BYTES, selection_struct, selection_dict)
_JOINT = _Rule("pose_support_joint", 3, JOINT_SEL_BYTES, joint_selection_struct, joint_selection_dict)


def _launch(rule, tracks, converge, scene, inliers, selections, flags, stream) -> None:
    """Enqueue hc_trifocal_<rule.name> on scene = (edgels, K), or its grouped
    form on scene = a multi.DeviceTripletBatch (no sync)."""
    grouped = not isinstance(scene, tuple)
    name = rule.name + ("_grouped" if grouped else "")
    n = converge.numel()
    T = scene.num_groups if grouped else 1
    if tracks.shape[0] != n or (grouped and n != scene.num_samples * _abi.NUM_TRACKS) or \
            inliers.numel() < rule.columns * n or selections.numel() < T * rule.sel_bytes:
        raise _abi.HCError(f"{name}: buffer sizes do not match")
    if grouped:
        for t in (tracks, converge, inliers, selections):
            if not t.is_cuda or not t.is_contiguous() or t.device != scene.target.device:
                raise _abi.HCError(f"{name}: buffers must be contiguous tensors on the batch's device")
        scene.check()   # group ids and edgel counts: the kernels do not validate them
        scene_args = (T, scene.groups, scene.sample_group)
    else:
        for t in (tracks, converge, *scene, inliers, selections):
            if not t.is_cuda or not t.is_contiguous():
                raise _abi.HCError(f"{name}: buffers must be contiguous device tensors")
        scene_args = (int(scene[0].shape[0]), *scene)
    args = [_abi.ptr(a) if isinstance(a, torch.Tensor) else a
            for a in (n, tracks, converge, *scene_args, flags, inliers, selections)]
    _abi.call("hc_trifocal_" + name, *args,
              _abi.ptr(stream if stream is not None else torch.cuda.current_stream(tracks.device)))


def _run(rule, tracks, converge, scene, flags=0):
    """Synchronous call on fresh buffers: (inliers (n, columns) numpy, the T
    selection dicts, the selections' device bytes)."""
    if not isinstance(scene, tuple) and not hasattr(scene, "groups"):
        scene = scene.to(tracks.device)
    dev = tracks.device
    n = converge.numel()
    T = 1 if isinstance(scene, tuple) else scene.num_groups
    inl = torch.empty((n, rule.columns), dtype=torch.int32, device=dev)
    sel = torch.empty(T * rule.sel_bytes, dtype=torch.uint8, device=dev)
    _launch(rule, tracks, converge, scene, inl, sel, flags, None)
    torch.cuda.synchronize(dev)
    raw = sel.cpu().numpy().reshape(T, rule.sel_bytes)
    return inl.cpu().numpy(), [rule.to_dict(rule.struct(r)) for r in raw], sel


def launch_pose_support(tracks: torch.Tensor, converge: torch.Tensor, edgels: torch.Tensor, K: torch.Tensor,
                        inliers: torch.Tensor, selection: torch.Tensor, quirks: bool = False, stream=None) -> None:
    """Enqueue candidate filter + pose + inlier scoring + selection (no sync).
    tracks (n, 31, 2) f32, converge (n,) u8, edgels (E, 6) f32, K (9,) f32 on the
    same device; inliers (n, 2) i32 and selection (SEL_BYTES,) u8 are outputs."""
    _launch(_PER_VIEW, tracks, converge, (edgels, K), inliers, selection,
            _abi.HC_POSE_REFERENCE_QUIRKS if quirks else 0, stream)


def pose_support(tracks: torch.Tensor, converge: torch.Tensor, data_edgels: torch.Tensor, K: torch.Tensor,
                 quirks: bool = False):
    """Synchronous wrapper: returns (inliers (n, 2) numpy, selection dict)."""
    inl, sels, _ = _run(_PER_VIEW, tracks, converge, (data_edgels, K), _abi.HC_POSE_REFERENCE_QUIRKS if quirks else 0)
    return inl, sels[0]


def launch_pose_support_grouped(tracks: torch.Tensor, converge: torch.Tensor, batch, inliers: torch.Tensor,
                                selections: torch.Tensor, stream=None) -> None:
    """Enqueue the pose support of several triplets' samples in one call (no
    sync): hc_trifocal_pose_support_grouped.  batch is a
    multi.DeviceTripletBatch; tracks / converge cover its samples in its order;
    selections (T * SEL_BYTES,) u8 receives one hcPoseSelection per triplet."""
    _launch(_PER_VIEW, tracks, converge, batch, inliers, selections, 0, stream)


def pose_support_grouped(tracks: torch.Tensor, converge: torch.Tensor, batch):
    """Synchronous wrapper: returns (inliers (n, 2) numpy, [selection dict] * T).
    Paths in the selections are the call's batch ids."""
    return _run(_PER_VIEW, tracks, converge, batch)[:2]


def launch_pose_support_joint(tracks: torch.Tensor, converge: torch.Tensor, edgels: torch.Tensor, K: torch.Tensor,
                              inliers: torch.Tensor, selection: torch.Tensor, stream=None) -> None:
    """Enqueue candidate filter + pose + joint inlier scoring + selection (no
    sync): hc_trifocal_pose_support_joint.  Buffers as in launch_pose_support,
    but inliers is (n, 3) i32 (joint, 21, 31) and selection (JOINT_SEL_BYTES,) u8."""
    _launch(_JOINT, tracks, converge, (edgels, K), inliers, selection, 0, stream)


def pose_support_joint(tracks: torch.Tensor, converge: torch.Tensor, data_edgels: torch.Tensor, K: torch.Tensor,
                       return_device_selection: bool = False):
    """Synchronous wrapper: returns (inliers (n, 3) numpy, selection dict), and
    with return_device_selection also the selection's device bytes (the input of
    inlier_mask)."""
    inl, sels, sel_dev = _run(_JOINT, tracks, converge, (data_edgels, K))
    return (inl, sels[0], sel_dev) if return_device_selection else (inl, sels[0])


def launch_pose_support_joint_grouped(tracks: torch.Tensor, converge: torch.Tensor, batch, inliers: torch.Tensor,
                                      selections: torch.Tensor, stream=None) -> None:
    """launch_pose_support_grouped with the joint rule
    (hc_trifocal_pose_support_joint_grouped): inliers (n, 3) i32, selections
    (T * JOINT_SEL_BYTES,) u8."""
    _launch(_JOINT, tracks, converge, batch, inliers, selections, 0, stream)


def pose_support_joint_grouped(tracks: torch.Tensor, converge: torch.Tensor, batch):
    """Synchronous wrapper: returns (inliers (n, 3) numpy, [selection dict] * T).
    Paths in the selections are the call's batch ids."""
    return _run(_JOINT, tracks, converge, batch)[:2]


def merge(parts: list, path_offsets: list, quirks: bool = False) -> dict:
    """hc_pose_merge: per-GPU selections (raw bytes or structs) with their first
    batch ids -> one selection with global batch ids."""
    n = len(parts)
    arr = (_abi.hcPoseSelection * max(1, n))()
    for i, p in enumerate(parts):
        arr[i] = p if isinstance(p, _abi.hcPoseSelection) else selection_struct(p)
    offs = np.ascontiguousarray(path_offsets, np.int32)
    out = _abi.hcPoseSelection()
    _abi.lib().hc_pose_merge(n, C.cast(arr, C.c_void_p), _abi.ptr(offs),
                             _abi.HC_POSE_REFERENCE_QUIRKS if quirks else 0, C.byref(out))
    return selection_dict(out)


def inlier_mask(selection, edgels: torch.Tensor, K: torch.Tensor, packed: bool = False, stream=None) -> np.ndarray:
    """hc_trifocal_pose_inlier_mask: which of the E edgels are within 2 px in
    both views under the selection's pose.  selection: the device bytes of an
    hcTrifocalSelection, or a struct / dict (e.g. a merge_joint result), which is
    uploaded.  Returns a bool array of length E, or with packed the (E + 63) // 64
    uint64 words."""
    dev = edgels.device
    if isinstance(selection, dict):
        selection = joint_selection_from_dict(selection)
    if isinstance(selection, _abi.hcTrifocalSelection):
        selection = torch.from_numpy(np.frombuffer(bytes(selection), np.uint8).copy()).to(dev)
    E = int(edgels.shape[0])
    for t in (selection, edgels, K):
        if not t.is_cuda or not t.is_contiguous() or t.device != dev:
            raise _abi.HCError("inlier_mask: buffers must be contiguous tensors on one device")
    if selection.numel() * selection.element_size() < JOINT_SEL_BYTES:
        raise _abi.HCError("inlier_mask: selection is smaller than hcTrifocalSelection")
    words = torch.empty((E + 63) // 64, dtype=torch.int64, device=dev)
    _abi.call("hc_trifocal_pose_inlier_mask", _abi.ptr(selection), E, _abi.ptr(edgels), _abi.ptr(K), _abi.ptr(words),
              _abi.ptr(stream if stream is not None else torch.cuda.current_stream(dev)))
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    w = words.cpu().numpy().view(np.uint64)
    if packed:
        return w
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:E].astype(bool)


# ---- refinement of a joint selection (include/refine/hc_pose_refine.h) --------
REPORT_BYTES = _abi.REFINE_REPORT_BYTES


def refine_report_dict(raw) -> dict:
    r = _struct_from_raw(_abi.hcRefineReport, REPORT_BYTES, raw)
    return dict(status=r.status, none=bool(r.status & _abi.HC_REFINE_NONE),
                too_few=bool(r.status & _abi.HC_REFINE_TOO_FEW), singular=bool(r.status & _abi.HC_REFINE_SINGULAR),
                iterations_run=r.iterations_run, best_iteration=r.best_iteration,
                joint_history=np.array(r.joint_history[:], np.int32),
                rms_px_in=np.array(r.rms_px_in[:], np.float64), rms_px_out=np.array(r.rms_px_out[:], np.float64))


def _device_selections(selections, dev, count: int, what: str) -> torch.Tensor:
    """count joint selections as device bytes: a uint8 device tensor as it is;
    a dict or struct, or a list of them, uploaded."""
    if not isinstance(selections, torch.Tensor):
        items = selections if isinstance(selections, (list, tuple)) else [selections]
        structs = [joint_selection_from_dict(s) if isinstance(s, dict) else joint_selection_struct(s) for s in items]
        raw = b"".join(bytes(s) for s in structs)
        selections = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
    if not selections.is_cuda or not selections.is_contiguous() or selections.device != dev:
        raise _abi.HCError(f"{what}: buffers must be contiguous tensors on one device")
    if selections.numel() * selections.element_size() < count * JOINT_SEL_BYTES:
        raise _abi.HCError(f"{what}: {count} hcTrifocalSelection expected")
    return selections


def _refine_settings(iterations, min_inliers, what: str) -> _abi.hcRefineSettings:
    """The explicit values of the Python interface (the header's 0 = default is
    not offered here: 0 iterations is refused, as every other value it would refuse)."""
    for v in (iterations, min_inliers):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise _abi.HCError(f"{what}: iterations and min_inliers must be integers")
    if not 1 <= iterations <= _abi.HC_REFINE_MAX_ITERATIONS:
        raise _abi.HCError(f"{what}: iterations {iterations} outside 1..{_abi.HC_REFINE_MAX_ITERATIONS}")
    if min_inliers < 6:
        raise _abi.HCError(f"{what}: min_inliers {min_inliers} below 6")
    s = _abi.hcRefineSettings()
    s.iterations, s.min_inliers = int(iterations), int(min_inliers)
    return s


# ---- the scale fit, a mode of the refine calls (include/scale/hc_pose_scale.h) ----
SCALE_REPORT_BYTES = _abi.SCALE_REPORT_BYTES


def scale_report_dict(raw) -> dict:
    r = _struct_from_raw(_abi.hcScaleReport, SCALE_REPORT_BYTES, raw)
    return dict(status=r.status, none=bool(r.status & _abi.HC_SCALE_NONE),
                no_voter=bool(r.status & _abi.HC_SCALE_NO_VOTER), num_voters=r.num_voters, voter=r.voter,
                transfer_inliers=r.transfer_inliers, tested=r.tested, joint=r.joint,
                scale_in=np.float32(r.scale_in), scale31=np.float32(r.scale31), key=r.key)


def _scale_report_dicts(raw: torch.Tensor, count: int) -> list:
    rows = raw.cpu().numpy().reshape(count, SCALE_REPORT_BYTES)
    return [scale_report_dict(r) for r in rows]


def _mask_words(words: torch.Tensor) -> np.ndarray:
    return words.cpu().numpy().view(np.uint64)


def _check_scale_flags(what: str, fit_scale, transfer_mask=False, select_by_transfer=False, mask_allowed=True):
    """The scale keywords of a refine wrapper, checked before anything touches a device."""
    for v in (fit_scale, transfer_mask, select_by_transfer):
        if not isinstance(v, (bool, np.bool_)):
            raise _abi.HCError(f"{what}: fit_scale, transfer_mask and select_by_transfer must be booleans")
    if not fit_scale and (transfer_mask or select_by_transfer):
        raise _abi.HCError(f"{what}: transfer_mask and select_by_transfer need fit_scale")
    if transfer_mask and not mask_allowed:
        raise _abi.HCError(f"{what}: the transfer mask is written for one scene only, not by the grouped call")


def _settings_ptr(settings):
    """The hcRefineSettings pointer of settings, or of an extended settings struct's head."""
    return C.cast(C.pointer(settings), C.POINTER(_abi.hcRefineSettings))


# ---- the three-view refinement, a further mode (include/threeview/hc_pose_threeview.h) ----
THREEVIEW_REPORT_BYTES = _abi.THREEVIEW_REPORT_BYTES


def three_view_report_dict(raw) -> dict:
    r = _struct_from_raw(_abi.hcThreeViewReport, THREEVIEW_REPORT_BYTES, raw)
    return dict(status=r.status, none=bool(r.status & _abi.HC_THREEVIEW_NONE),
                too_few=bool(r.status & _abi.HC_THREEVIEW_TOO_FEW),
                singular=bool(r.status & _abi.HC_THREEVIEW_SINGULAR),
                skipped=bool(r.status & _abi.HC_THREEVIEW_SKIPPED),
                iterations_run=r.iterations_run, best_iteration=r.best_iteration,
                transfer_history=np.array(r.transfer_history[:], np.int32),
                joint_history=np.array(r.joint_history[:], np.int32),
                fit_set=r.fit_set, transfer_inliers=r.transfer_inliers,
                scale_in=np.float32(r.scale_in), scale_out=np.float32(r.scale_out),
                rms_px_in=np.array(r.rms_px_in[:], np.float64), rms_px_out=np.array(r.rms_px_out[:], np.float64))


def _three_view_report_dicts(raw: torch.Tensor, count: int) -> list:
    rows = raw.cpu().numpy().reshape(count, THREEVIEW_REPORT_BYTES)
    return [three_view_report_dict(r) for r in rows]


def _check_three_view(what: str, three_view, three_view_iterations, fit_scale):
    """The three-view keywords of a refine wrapper, checked before anything
    touches a device.  Returns fit_scale, which three_view implies."""
    if not isinstance(three_view, (bool, np.bool_)):
        raise _abi.HCError(f"{what}: three_view must be a boolean")
    if three_view_iterations is not None:
        v = three_view_iterations
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or \
                not 1 <= v <= _abi.HC_REFINE_MAX_ITERATIONS:
            raise _abi.HCError(f"{what}: three_view_iterations {v!r} outside 1..{_abi.HC_REFINE_MAX_ITERATIONS}")
        if not three_view:
            raise _abi.HCError(f"{what}: three_view_iterations needs three_view")
    if three_view and not isinstance(fit_scale, (bool, np.bool_)):
        raise _abi.HCError(f"{what}: fit_scale must be a boolean")
    return True if three_view else fit_scale


def _three_view_mode(settings, count: int, dev, three_view_iterations, transfer_mask=False, num_edgels=None,
                     select_by_transfer=False):
    """An hcRefineThreeViewSettings with `settings` as its head, count scale
    reports and count three-view reports and, with transfer_mask, the mask's
    words (new device tensors).  Returns (settings, scale reports, mask words or
    None, three-view reports)."""
    ts = _abi.hcRefineThreeViewSettings()
    ts.head.iterations, ts.head.min_inliers = settings.iterations, settings.min_inliers
    ts.head.pad[0] = _abi.HC_REFINE_THREEVIEW
    ts.head.pad[1] = _abi.HC_THREEVIEW_SELECT_BY_TRANSFER if select_by_transfer else 0
    scale = torch.empty(count * SCALE_REPORT_BYTES, dtype=torch.uint8, device=dev)
    reports = torch.empty(count * THREEVIEW_REPORT_BYTES, dtype=torch.uint8, device=dev)
    words = torch.empty((num_edgels + 63) // 64, dtype=torch.int64, device=dev) if transfer_mask else None
    ts.scale_reports, ts.reports = scale.data_ptr(), reports.data_ptr()
    ts.transfer_mask = words.data_ptr() if words is not None else None
    ts.iterations3 = 10 if three_view_iterations is None else int(three_view_iterations)
    return ts, scale, words, reports


# ---- the 3D edgels, a further mode (include/structure/hc_pose_structure.h) ----
EDGEL3D_BYTES = _abi.EDGEL3D_BYTES
EDGEL3D_DTYPE = _abi.EDGEL3D_DTYPE
STRUCTURE_REPORT_BYTES = _abi.STRUCTURE_REPORT_BYTES


def structure_report_dict(raw) -> dict:
    r = _struct_from_raw(_abi.hcStructureReport, STRUCTURE_REPORT_BYTES, raw)
    return dict(status=r.status, none=bool(r.status & _abi.HC_STRUCTURE_NONE), count=r.count, tangents=r.tangents,
                oriented=r.oriented, scale31=np.float32(r.scale31))


def _structure_report_dicts(raw: torch.Tensor, count: int) -> list:
    rows = raw.cpu().numpy().reshape(count, STRUCTURE_REPORT_BYTES)
    return [structure_report_dict(r) for r in rows]


def structure_records(edgels3d: torch.Tensor, report: dict, first: int = 0) -> np.ndarray:
    """The report's first `count` hcEdgel3D of a device buffer, from entry
    `first`, as a structured array (EDGEL3D_DTYPE)."""
    rec = edgels3d.cpu().numpy().view(np.uint8).reshape(-1).view(EDGEL3D_DTYPE)
    return rec[first:first + report["count"]].copy()


def _check_structure(what: str, structure, tangents, min_sin_plane, max_sin3, three_view):
    """The structure keywords of a refine wrapper, checked before anything
    touches a device.  Returns three_view, which structure implies."""
    if not isinstance(structure, (bool, np.bool_)):
        raise _abi.HCError(f"{what}: structure must be a boolean")
    if not structure:
        if tangents is not None:
            raise _abi.HCError(f"{what}: tangents need structure")
        return three_view
    if not isinstance(three_view, (bool, np.bool_)):
        raise _abi.HCError(f"{what}: three_view must be a boolean")
    for v in (min_sin_plane, max_sin3):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or not 0.0 < float(v) <= 1.0:
            raise _abi.HCError(f"{what}: min_sin_plane and max_sin3 must lie in (0, 1], not {v!r}")
    return True


def _structure_mode(ts, what: str, dev, tangents, num_edgels: int, min_sin_plane, max_sin3, groups: int = 1,
                    edgel_offsets=None, edgels3d=None):
    """An hcRefineStructureSettings around the three-view settings ts (None:
    HC_STRUCTURE_ONLY), the tangents of num_edgels edgels in all, and new device
    tensors for the records (unless edgels3d is given) and the `groups` reports.
    Returns (settings, records (num_edgels * EDGEL3D_BYTES,) u8, reports)."""
    if not isinstance(tangents, torch.Tensor) or tangents.dtype != torch.float32 or not tangents.is_cuda or \
            not tangents.is_contiguous() or tangents.device != dev or tangents.numel() != 6 * num_edgels:
        raise _abi.HCError(f"{what}: tangents must be a contiguous float32 ({num_edgels}, 6) tensor on the scene's device")
    ss = _abi.hcRefineStructureSettings()
    if ts is not None:
        ss.tv = ts
        bits = ts.head.pad[1]
    else:
        bits = _abi.HC_STRUCTURE_ONLY
    ss.tv.head.pad[0], ss.tv.head.pad[1] = _abi.HC_REFINE_STRUCTURE, bits
    if edgels3d is None:
        edgels3d = torch.empty(num_edgels * EDGEL3D_BYTES, dtype=torch.uint8, device=dev)
    if not edgels3d.is_cuda or not edgels3d.is_contiguous() or edgels3d.device != dev or \
            edgels3d.numel() * edgels3d.element_size() < num_edgels * EDGEL3D_BYTES:
        raise _abi.HCError(f"{what}: edgels3d must hold {num_edgels} hcEdgel3D on the scene's device")
    reports = torch.empty(groups * STRUCTURE_REPORT_BYTES, dtype=torch.uint8, device=dev)
    ss.tangents, ss.edgels3d, ss.reports = tangents.data_ptr(), edgels3d.data_ptr(), reports.data_ptr()
    ss.edgel_offsets = edgel_offsets.data_ptr() if edgel_offsets is not None else None
    ss.min_sin_plane, ss.max_sin3 = float(min_sin_plane), float(max_sin3)
    return ss, edgels3d, reports


def write_edgels3d(path: str, structure: np.ndarray) -> None:
    """One text line per record: edgel X T err3_px sin_plane sin3 flags, floats as %.9g."""
    with open(path, "w") as fh:
        for r in np.asarray(structure, EDGEL3D_DTYPE).reshape(-1):
            vals = [*r["X"], *r["T"], r["err3_px"], r["sin_plane"], r["sin3"]]
            fh.write(f"{int(r['edgel'])} " + " ".join("%.9g" % float(v) for v in vals) + f" {int(r['flags'])}\n")


def _scale_mode(settings, count: int, dev, what: str, fit_scale, transfer_mask=False, num_edgels=None,
                select_by_transfer=False, scale_only=False):
    """The settings a refine call is given: `settings` itself with the mode off,
    otherwise an hcRefineScaleSettings with `settings` as its head, count scale
    reports and, with transfer_mask, the mask's words (new device tensors).
    Returns (settings, scale reports or None, mask words or None)."""
    _check_scale_flags(what, fit_scale, transfer_mask, select_by_transfer, num_edgels is not None)
    if not fit_scale:
        return settings, None, None
    ss = _abi.hcRefineScaleSettings()
    ss.head.iterations, ss.head.min_inliers = (0 if scale_only else settings.iterations), settings.min_inliers
    ss.head.pad[0] = _abi.HC_REFINE_SCALE31
    ss.head.pad[1] = (_abi.HC_SCALE_ONLY if scale_only else 0) | \
        (_abi.HC_SCALE_SELECT_BY_TRANSFER if select_by_transfer else 0)
    reports = torch.empty(count * SCALE_REPORT_BYTES, dtype=torch.uint8, device=dev)
    words = torch.empty((num_edgels + 63) // 64, dtype=torch.int64, device=dev) if transfer_mask else None
    ss.reports = reports.data_ptr()
    ss.transfer_mask = words.data_ptr() if words is not None else None
    return ss, reports, words


def launch_refine_joint(selection, edgels: torch.Tensor, K: torch.Tensor, iterations: int = 10,
                        min_inliers: int = 16, stream=None, out: torch.Tensor | None = None,
                        fit_scale: bool = False, transfer_mask: bool = False, _scale_only: bool = False,
                        three_view: bool = False, three_view_iterations: int | None = None,
                        structure: bool = False, tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05,
                        max_sin3: float = 0.05, edgels3d: torch.Tensor | None = None, _structure_only: bool = False):
    """Enqueue hc_trifocal_pose_refine (no sync): the joint selection's pose
    fitted to its joint inliers among the E edgels, the inlier set recomputed at
    every iterate.  selection: the device bytes of an hcTrifocalSelection, or a
    dict / struct (e.g. a merge_joint result), which is uploaded.  out: the
    device bytes to write (may be selection itself); default a new tensor.
    Returns (refined selection (JOINT_SEL_BYTES,) u8, report (REPORT_BYTES,) u8),
    both on the device.
    fit_scale: the refined pose's scale31 is fitted by three-view transfer
    support in the same call (include/scale/hc_pose_scale.h); two more device
    tensors are returned, the scale report (SCALE_REPORT_BYTES,) u8 and, with
    transfer_mask, the transfer mask's (E + 63) // 64 int64 words (else None).
    three_view: after the fit, both views and the scale are refined jointly on
    the three-view transfer for three_view_iterations steps (default 10;
    include/threeview/hc_pose_threeview.h).  It implies fit_scale; a fifth
    device tensor is returned, the three-view report (THREEVIEW_REPORT_BYTES,)
    u8, and the transfer mask describes the pose and scale that went out.
    structure: after the three-view stage, which it implies, the 3D edgels the
    pose that went out explains are reconstructed from tangents (E, 6) f32
    (include/structure/hc_pose_structure.h); two more device tensors follow, the
    records (E * EDGEL3D_BYTES,) u8 (a new tensor unless edgels3d is given; the
    report's count of them are written) and the structure report
    (STRUCTURE_REPORT_BYTES,) u8."""
    what = "refine_joint"
    settings = _refine_settings(iterations, min_inliers, what)
    three_view = _check_structure(what, structure, tangents, min_sin_plane, max_sin3, three_view)
    fit_scale = _check_three_view(what, three_view, three_view_iterations, fit_scale)
    _check_scale_flags(what, fit_scale, transfer_mask)
    dev = edgels.device
    selection = _device_selections(selection, dev, 1, what)
    for t in (edgels, K):
        if not t.is_cuda or not t.is_contiguous() or t.device != dev:
            raise _abi.HCError(f"{what}: buffers must be contiguous tensors on one device")
    if out is None:
        out = torch.empty(JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    out = _device_selections(out, dev, 1, what)
    tv = None
    if _structure_only:
        scale = words = None
        settings, rec, srep = _structure_mode(None, what, dev, tangents, int(edgels.shape[0]), min_sin_plane, max_sin3,
                                              edgels3d=edgels3d)
    elif three_view:
        settings, scale, words, tv = _three_view_mode(settings, 1, dev, three_view_iterations, transfer_mask,
                                                      int(edgels.shape[0]))
        if structure:
            settings, rec, srep = _structure_mode(settings, what, dev, tangents, int(edgels.shape[0]), min_sin_plane,
                                                  max_sin3, edgels3d=edgels3d)
    else:
        settings, scale, words = _scale_mode(settings, 1, dev, what, fit_scale, transfer_mask, int(edgels.shape[0]),
                                             scale_only=_scale_only)
    report = None if _scale_only or _structure_only else torch.empty(REPORT_BYTES, dtype=torch.uint8, device=dev)
    _abi.call("hc_trifocal_pose_refine", _abi.ptr(selection), int(edgels.shape[0]), _abi.ptr(edgels), _abi.ptr(K),
              _settings_ptr(settings), _abi.ptr(out), _abi.ptr(report),
              _abi.ptr(stream if stream is not None else torch.cuda.current_stream(dev)))
    if structure:
        return out, report, scale, words, tv, rec, srep
    if three_view:
        return out, report, scale, words, tv
    return (out, report, scale, words) if fit_scale else (out, report)


def _scale_entry(scale: torch.Tensor, words) -> dict:
    d = scale_report_dict(scale)
    if words is not None:
        d["mask"] = _mask_words(words)
    return d


def refine_joint(selection, edgels: torch.Tensor, K: torch.Tensor, iterations: int = 10, min_inliers: int = 16,
                 return_device_selection: bool = False, fit_scale: bool = False, transfer_mask: bool = False,
                 three_view: bool = False, three_view_iterations: int | None = None, structure: bool = False,
                 tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Synchronous wrapper: (refined selection dict, report dict), and with
    return_device_selection also the refined selection's device bytes.  With
    fit_scale the report dict has a "scale" entry, the scale report as a dict
    (with transfer_mask also its "mask", the packed uint64 words).  With
    three_view it has both "scale" (the vote's report) and "three_view" (the
    three-view report as a dict, which then holds "mask").  With structure
    (which implies three_view) it also has "structure", the structure report as
    a dict, and the records follow the report dict: (selection dict, report
    dict, structure), structure a structured array of EDGEL3D_DTYPE."""
    out, report, *rest = launch_refine_joint(selection, edgels, K, iterations, min_inliers, fit_scale=fit_scale,
                                             transfer_mask=transfer_mask, three_view=three_view,
                                             three_view_iterations=three_view_iterations, structure=structure,
                                             tangents=tangents, min_sin_plane=min_sin_plane, max_sin3=max_sin3)
    torch.cuda.synchronize(edgels.device)
    rep = refine_report_dict(report)
    three_view = three_view or structure
    if three_view:
        rep["scale"] = scale_report_dict(rest[0])
        rep["three_view"] = three_view_report_dict(rest[2])
        if rest[1] is not None:
            rep["three_view"]["mask"] = _mask_words(rest[1])
    elif fit_scale:
        rep["scale"] = _scale_entry(*rest)
    res = (joint_selection_dict(joint_selection_struct(out)), rep)
    if structure:
        rep["structure"] = structure_report_dict(rest[4])
        res = (*res, structure_records(rest[3], rep["structure"]))
    return (*res, out) if return_device_selection else res


def launch_reconstruct(selection, edgels: torch.Tensor, tangents: torch.Tensor, K: torch.Tensor,
                       min_sin_plane: float = 0.05, max_sin3: float = 0.05, stream=None,
                       out: torch.Tensor | None = None, edgels3d: torch.Tensor | None = None):
    """Enqueue the reconstruction alone (hc_trifocal_pose_refine with
    HC_STRUCTURE_ONLY, no sync): nothing is refined or voted, the 3D edgels are
    those of the selection's own pose and scale31.  Returns device tensors
    (selection, a bit-for-bit copy; records (E * EDGEL3D_BYTES,) u8; structure
    report (STRUCTURE_REPORT_BYTES,) u8)."""
    o, *_, rec, srep = launch_refine_joint(selection, edgels, K, stream=stream, out=out, structure=True,
                                           tangents=tangents, min_sin_plane=min_sin_plane, max_sin3=max_sin3,
                                           edgels3d=edgels3d, _structure_only=True)
    return o, rec, srep


def reconstruct(selection, edgels: torch.Tensor, tangents: torch.Tensor, K: torch.Tensor, min_sin_plane: float = 0.05,
                max_sin3: float = 0.05):
    """The 3D edgels a selection's pose and scale31 explain, synchronous:
    (structure, report): the report's count records in edgel order as a
    structured array of EDGEL3D_DTYPE, and the structure report as a dict."""
    _, rec, srep = launch_reconstruct(selection, edgels, tangents, K, min_sin_plane, max_sin3)
    torch.cuda.synchronize(edgels.device)
    report = structure_report_dict(srep)
    return structure_records(rec, report), report


def launch_fit_scale31(selection, edgels: torch.Tensor, K: torch.Tensor, transfer_mask: bool = False, stream=None,
                       out: torch.Tensor | None = None):
    """Enqueue the scale fit alone (hc_trifocal_pose_refine with HC_SCALE_ONLY,
    no sync): no Gauss-Newton step, the selection comes back with only scale31
    replaced.  Returns device tensors (selection, scale report, mask words or None)."""
    o, _, scale, words = launch_refine_joint(selection, edgels, K, stream=stream, out=out, fit_scale=True,
                                             transfer_mask=transfer_mask, _scale_only=True)
    return o, scale, words


def fit_scale31(selection, edgels: torch.Tensor, K: torch.Tensor, transfer_mask: bool = False):
    """The scale-only form, synchronous: (selection dict, scale report dict)."""
    out, scale, words = launch_fit_scale31(selection, edgels, K, transfer_mask)
    torch.cuda.synchronize(edgels.device)
    return joint_selection_dict(joint_selection_struct(out)), _scale_entry(scale, words)


def launch_refine_joint_grouped(selections, batch, iterations: int = 10, min_inliers: int = 16, stream=None,
                                fit_scale: bool = False, transfer_mask: bool = False, three_view: bool = False,
                                three_view_iterations: int | None = None, structure: bool = False,
                                tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05,
                                max_sin3: float = 0.05, edgels3d: torch.Tensor | None = None,
                                _structure_only: bool = False):
    """Enqueue hc_trifocal_pose_refine_grouped (no sync): selection t refined on
    triplet t of batch (a multi.DeviceTripletBatch).  selections: T selections
    as device bytes, or a list of dicts / structs, which is uploaded.  Returns
    (selections (T * JOINT_SEL_BYTES,) u8, reports (T * REPORT_BYTES,) u8), and
    with fit_scale also the scale reports (T * SCALE_REPORT_BYTES,) u8.  The
    grouped call writes no transfer mask: transfer_mask is refused.  With
    three_view (which implies fit_scale) a fourth tensor follows, the three-view
    reports (T * THREEVIEW_REPORT_BYTES,) u8.  With structure (which implies
    three_view) two more follow: the records of all triplets (sum E *
    EDGEL3D_BYTES,) u8, triplet t's from entry batch.edgel_offsets[t], and
    the T structure reports.  tangents: the batch's own unless given."""
    what = "refine_joint_grouped"
    settings = _refine_settings(iterations, min_inliers, what)
    three_view = _check_structure(what, structure, tangents, min_sin_plane, max_sin3, three_view)
    fit_scale = _check_three_view(what, three_view, three_view_iterations, fit_scale)
    _check_scale_flags(what, fit_scale, transfer_mask, mask_allowed=False)
    dev = batch.device
    T = batch.num_groups
    if not isinstance(selections, torch.Tensor) and len(selections) != T:
        raise _abi.HCError(f"{what}: {len(selections)} selections for {T} triplets")
    selections = _device_selections(selections, dev, T, what)
    batch.check()   # edgel counts: the kernel does not validate them
    out = torch.empty(T * JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    reports = torch.empty(T * REPORT_BYTES, dtype=torch.uint8, device=dev)
    tv = None
    sm = (what, dev, batch.tangents if tangents is None else tangents, int(batch.edgels.shape[0]), min_sin_plane,
          max_sin3, T, batch.edgel_offsets_device, edgels3d) if structure else None
    if _structure_only:
        scale, reports = None, None
        settings, rec, srep = _structure_mode(None, *sm)
    elif three_view:
        settings, scale, _, tv = _three_view_mode(settings, T, dev, three_view_iterations)
        if structure:
            settings, rec, srep = _structure_mode(settings, *sm)
    else:
        settings, scale, _ = _scale_mode(settings, T, dev, what, fit_scale, transfer_mask)
    _abi.call("hc_trifocal_pose_refine_grouped", T, _abi.ptr(batch.groups), _abi.ptr(selections),
              _settings_ptr(settings), _abi.ptr(out), _abi.ptr(reports),
              _abi.ptr(stream if stream is not None else torch.cuda.current_stream(dev)))
    if structure:
        return out, reports, scale, tv, rec, srep
    if three_view:
        return out, reports, scale, tv
    return (out, reports, scale) if fit_scale else (out, reports)


def refine_joint_grouped(selections, batch, iterations: int = 10, min_inliers: int = 16, device=None,
                         fit_scale: bool = False, transfer_mask: bool = False, three_view: bool = False,
                         three_view_iterations: int | None = None, structure: bool = False,
                         tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Synchronous wrapper: ([refined selection dict] * T, [report dict] * T).
    batch: a multi.TripletBatch (copied to device, or to the selections' device)
    or a multi.DeviceTripletBatch.  With fit_scale every report dict has a
    "scale" entry, with three_view also a "three_view" entry.  With structure
    (which implies three_view) also a "structure" entry, and a third list
    follows, every triplet's records."""
    three_view = _check_structure("refine_joint_grouped", structure, tangents, min_sin_plane, max_sin3, three_view)
    fit_scale = _check_three_view("refine_joint_grouped", three_view, three_view_iterations, fit_scale)
    _check_scale_flags("refine_joint_grouped", fit_scale, transfer_mask, mask_allowed=False)
    if not hasattr(batch, "groups"):
        if device is None:
            device = selections.device if isinstance(selections, torch.Tensor) else "cuda:0"
        batch = batch.to(device)
    out, reports, *rest = launch_refine_joint_grouped(selections, batch, iterations, min_inliers, fit_scale=fit_scale,
                                                      transfer_mask=transfer_mask, three_view=three_view,
                                                      three_view_iterations=three_view_iterations, structure=structure,
                                                      tangents=tangents, min_sin_plane=min_sin_plane, max_sin3=max_sin3)
    torch.cuda.synchronize(batch.device)
    T = batch.num_groups
    sels = out.cpu().numpy().reshape(T, JOINT_SEL_BYTES)
    reps = [refine_report_dict(r) for r in reports.cpu().numpy().reshape(T, REPORT_BYTES)]
    if fit_scale:
        for r, s in zip(reps, _scale_report_dicts(rest[0], T)):
            r["scale"] = s
    if three_view:
        for r, s in zip(reps, _three_view_report_dicts(rest[1], T)):
            r["three_view"] = s
    dicts = [joint_selection_dict(joint_selection_struct(r)) for r in sels]
    if structure:
        for r, s in zip(reps, _structure_report_dicts(rest[3], T)):
            r["structure"] = s
        return dicts, reps, _group_records(rest[2], reps, batch)
    return dicts, reps


def _group_records(edgels3d: torch.Tensor, structure_reports, batch) -> list:
    """Every triplet's records of a grouped call; structure_reports: dicts with
    a "structure" entry, or structure report dicts."""
    rec = edgels3d.cpu().numpy().view(np.uint8).reshape(-1).view(EDGEL3D_DTYPE)
    offs = batch.edgel_offsets
    return [rec[int(o):int(o) + r.get("structure", r)["count"]].copy() for o, r in zip(offs, structure_reports)]


def launch_reconstruct_grouped(selections, batch, tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05,
                               max_sin3: float = 0.05, stream=None, edgels3d: torch.Tensor | None = None):
    """launch_reconstruct for every triplet of batch (a
    multi.DeviceTripletBatch) in one call, hc_trifocal_pose_refine_grouped with
    HC_STRUCTURE_ONLY (no sync).  Returns device tensors (selections, copied bit
    for bit; the records of all triplets; the T structure reports)."""
    o, *_, rec, srep = launch_refine_joint_grouped(selections, batch, stream=stream, structure=True,
                                                   tangents=tangents, min_sin_plane=min_sin_plane,
                                                   max_sin3=max_sin3, edgels3d=edgels3d, _structure_only=True)
    return o, rec, srep


def reconstruct_grouped(selections, batch, tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05,
                        max_sin3: float = 0.05):
    """Synchronous: ([structure] * T, [report dict] * T)."""
    _, rec, srep = launch_reconstruct_grouped(selections, batch, tangents, min_sin_plane, max_sin3)
    torch.cuda.synchronize(batch.device)
    reports = _structure_report_dicts(srep, batch.num_groups)
    return _group_records(rec, reports, batch), reports


def merge_joint(parts: list, path_offsets: list) -> dict:
    """hc_pose_merge_joint: per-launch / per-GPU joint selections (raw bytes,
    structs or dicts) with their first batch ids -> one selection with global
    batch ids."""
    n = len(parts)
    arr = (_abi.hcTrifocalSelection * max(1, n))()
    for i, p in enumerate(parts):
        arr[i] = joint_selection_from_dict(p) if isinstance(p, dict) else joint_selection_struct(p)
    offs = np.ascontiguousarray(path_offsets if n else [0], np.int32)
    out = _abi.hcTrifocalSelection()
    _abi.lib().hc_pose_merge_joint(n, C.cast(arr, C.c_void_p), _abi.ptr(offs), C.byref(out))
    return joint_selection_dict(out)


# ---- the k best joint candidates, refined, and the selection among them -------
# (include/topk/hc_pose_topk.h)
TOPK_MAX = _abi.HC_TOPK_MAX


def _check_k(k, what: str) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= TOPK_MAX:
        raise _abi.HCError(f"{what}: k {k!r} outside 1..{TOPK_MAX}")
    return int(k)


def _selection_dicts(raw: torch.Tensor, count: int) -> list:
    rows = raw.cpu().numpy().view(np.uint8).reshape(-1)[:count * JOINT_SEL_BYTES].reshape(count, JOINT_SEL_BYTES)
    return [joint_selection_dict(joint_selection_struct(r)) for r in rows]


def _launch_topk(what, tracks, inliers, k, groups, sample_group, candidates, stream):
    k = _check_k(k, what)
    n = int(tracks.shape[0])
    dev = tracks.device
    if candidates is None:
        candidates = torch.empty(groups * k * JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    bufs = (tracks, inliers, candidates) + (() if sample_group is None else (sample_group,))
    for t in bufs:
        if not t.is_cuda or not t.is_contiguous() or t.device != dev:
            raise _abi.HCError(f"{what}: buffers must be contiguous tensors on one device")
    if inliers.numel() < 3 * n or candidates.numel() * candidates.element_size() < groups * k * JOINT_SEL_BYTES or \
            (sample_group is not None and sample_group.numel() * _abi.NUM_TRACKS != n):
        raise _abi.HCError(f"{what}: buffer sizes do not match")
    s = _abi.ptr(stream if stream is not None else torch.cuda.current_stream(dev))
    if sample_group is None:
        _abi.call("hc_trifocal_pose_topk_joint", n, _abi.ptr(tracks), _abi.ptr(inliers), k, _abi.ptr(candidates), s)
    else:
        _abi.call("hc_trifocal_pose_topk_joint_grouped", n, _abi.ptr(tracks), _abi.ptr(inliers), groups,
                  _abi.ptr(sample_group), k, _abi.ptr(candidates), s)
    return candidates


def launch_topk_joint(tracks: torch.Tensor, inliers: torch.Tensor, k: int, candidates: torch.Tensor | None = None,
                      stream=None) -> torch.Tensor:
    """Enqueue hc_trifocal_pose_topk_joint (no sync): the k candidates with the
    most joint inliers (ties -> the larger batch id), best first, from the (n, 3)
    counts a joint pose-support call has written.  Returns candidates, the device
    bytes of k hcTrifocalSelection (a new tensor unless given); ranks beyond the
    number of candidates are "none" selections."""
    return _launch_topk("topk_joint", tracks, inliers, k, 1, None, candidates, stream)


def topk_joint(tracks: torch.Tensor, inliers: torch.Tensor, k: int, return_device_selection: bool = False):
    """Synchronous wrapper: [selection dict] * k, and with
    return_device_selection also their device bytes."""
    cand = launch_topk_joint(tracks, inliers, k)
    torch.cuda.synchronize(tracks.device)
    dicts = _selection_dicts(cand, _check_k(k, "topk_joint"))
    return (dicts, cand) if return_device_selection else dicts


def launch_topk_joint_grouped(tracks: torch.Tensor, inliers: torch.Tensor, batch, k: int,
                              candidates: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Enqueue hc_trifocal_pose_topk_joint_grouped (no sync): per triplet t of
    batch (a multi.DeviceTripletBatch) the k best candidates among its own
    samples, at candidates[t * k + r], with the call's batch ids."""
    what = "topk_joint_grouped"
    _check_k(k, what)
    if tracks.shape[0] != batch.num_samples * _abi.NUM_TRACKS or tracks.device != batch.device:
        raise _abi.HCError(f"{what}: tracks do not cover the batch's samples on its device")
    batch.check()   # group ids: the kernel does not validate them
    return _launch_topk(what, tracks, inliers, k, batch.num_groups, batch.sample_group, candidates, stream)


def topk_joint_grouped(tracks: torch.Tensor, inliers: torch.Tensor, batch, k: int):
    """Synchronous wrapper: a list of T lists of k selection dicts.  batch: a
    multi.TripletBatch (copied to the tracks' device) or a multi.DeviceTripletBatch."""
    if not hasattr(batch, "groups"):
        batch = batch.to(tracks.device)
    cand = launch_topk_joint_grouped(tracks, inliers, batch, k)
    torch.cuda.synchronize(tracks.device)
    d = _selection_dicts(cand, batch.num_groups * k)
    return [d[t * k:(t + 1) * k] for t in range(batch.num_groups)]


def _launch_refine_topk(what, candidates, k, scene, iterations, min_inliers, stream, refined, fit_scale=False,
                        transfer_mask=False, select_by_transfer=False, three_view=False, three_view_iterations=None,
                        structure=False, tangents=None, min_sin_plane=0.05, max_sin3=0.05):
    """scene: (edgels, K) or a multi.DeviceTripletBatch.  With fit_scale the
    returned tuple has a fifth tensor, the T * k scale reports, and, when
    transfer_mask is set, a sixth: the transfer mask of best (the single-scene
    call only), written by a scale-only fit of best on the same stream.  With
    three_view the tuple is (best, best_rank, refined, reports, scale reports,
    three-view reports); a transfer mask is then refused (the scale-only fit of
    best would vote its scale again).  With structure (which implies
    three_view) two more tensors follow: the records of best (one scene: E;
    grouped: sum E, triplet t's from entry edgel_offsets[t]) and the T structure
    reports."""
    k = _check_k(k, what)
    settings = _refine_settings(iterations, min_inliers, what)
    three_view = _check_structure(what, structure, tangents, min_sin_plane, max_sin3, three_view)
    fit_scale = _check_three_view(what, three_view, three_view_iterations, fit_scale)
    if three_view and transfer_mask is True:
        raise _abi.HCError(f"{what}: with three_view the transfer mask is written by refine_joint only")
    grouped = not isinstance(scene, tuple)
    _check_scale_flags(what, fit_scale, transfer_mask, select_by_transfer, not grouped)
    dev = scene.device if grouped else scene[0].device
    T = scene.num_groups if grouped else 1
    if not isinstance(candidates, torch.Tensor) and len(candidates) != T * k:
        raise _abi.HCError(f"{what}: {len(candidates)} candidates for {T} x {k}")
    candidates = _device_selections(candidates, dev, T * k, what)
    if refined is None:
        refined = torch.empty(T * k * JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    refined = _device_selections(refined, dev, T * k, what)
    reports = torch.empty(T * k * REPORT_BYTES, dtype=torch.uint8, device=dev)
    best = torch.empty(T * JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    best_rank = torch.empty(T, dtype=torch.int32, device=dev)
    tv = None
    if three_view:
        settings, scale, _, tv = _three_view_mode(settings, T * k, dev, three_view_iterations,
                                                  select_by_transfer=select_by_transfer)
        if structure and grouped:
            settings, rec, srep = _structure_mode(settings, what, dev, scene.tangents if tangents is None else tangents,
                                                  int(scene.edgels.shape[0]), min_sin_plane, max_sin3, T,
                                                  scene.edgel_offsets_device)
        elif structure:
            settings, rec, srep = _structure_mode(settings, what, dev, tangents, int(scene[0].shape[0]),
                                                  min_sin_plane, max_sin3)
    else:
        settings, scale, _ = _scale_mode(settings, T * k, dev, what, fit_scale, select_by_transfer=select_by_transfer)
    s = _abi.ptr(stream if stream is not None else torch.cuda.current_stream(dev))
    out = (_abi.ptr(refined), _abi.ptr(reports), _abi.ptr(best), _abi.ptr(best_rank), s)
    if grouped:
        scene.check()   # edgel counts: the kernel does not validate them
        _abi.call("hc_trifocal_pose_refine_topk_grouped", T, _abi.ptr(scene.groups), k, _abi.ptr(candidates),
                  _settings_ptr(settings), *out)
    else:
        for t in scene:
            if not t.is_cuda or not t.is_contiguous() or t.device != dev:
                raise _abi.HCError(f"{what}: buffers must be contiguous tensors on one device")
        _abi.call("hc_trifocal_pose_refine_topk", k, _abi.ptr(candidates), int(scene[0].shape[0]), _abi.ptr(scene[0]),
                  _abi.ptr(scene[1]), _settings_ptr(settings), *out)
    if structure:
        return best, best_rank, refined, reports, scale, tv, rec, srep
    if three_view:
        return best, best_rank, refined, reports, scale, tv
    if not fit_scale:
        return best, best_rank, refined, reports
    if not transfer_mask:
        return best, best_rank, refined, reports, scale
    # the same pose gives the same vote: best keeps its bytes, and the mask is its own
    _, _, words = launch_fit_scale31(best, scene[0], scene[1], transfer_mask=True, stream=stream, out=best)
    return best, best_rank, refined, reports, scale, words


def _topk_extra(out: tuple, three_view: bool) -> tuple:
    """The (scale, words, three_view) arguments of _refine_topk_dicts from a launch's tuple."""
    return (out[4], None, out[5]) if three_view else out[4:]


def _topk_count(candidates, what: str) -> int:
    if isinstance(candidates, torch.Tensor):
        n, rem = divmod(candidates.numel() * candidates.element_size(), JOINT_SEL_BYTES)
        if rem:
            raise _abi.HCError(f"{what}: the candidates are not a whole number of hcTrifocalSelection")
        return n
    return len(candidates)


def launch_refine_topk(candidates, edgels: torch.Tensor, K: torch.Tensor, iterations: int = 10, min_inliers: int = 16,
                       stream=None, refined: torch.Tensor | None = None, fit_scale: bool = False,
                       transfer_mask: bool = False, select_by_transfer: bool = False, three_view: bool = False,
                       three_view_iterations: int | None = None, structure: bool = False,
                       tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Enqueue hc_trifocal_pose_refine_topk (no sync): every candidate refined
    on the E edgels as launch_refine_joint refines it, in one launch, and the
    refined selection with the most joint inliers (ties -> the larger batch id)
    selected.  candidates: the device bytes of k hcTrifocalSelection (the output
    of launch_topk_joint: k is their number), or a list of k dicts / structs,
    which is uploaded.  refined: the device bytes to write (may be candidates).
    Returns device tensors (best (JOINT_SEL_BYTES,) u8, best_rank (1,) i32,
    refined (k * JOINT_SEL_BYTES,) u8, reports (k * REPORT_BYTES,) u8).
    fit_scale: the scale31 of all k refined selections is fitted by three-view
    transfer support (include/scale/hc_pose_scale.h) and a fifth tensor, the k
    scale reports (k * SCALE_REPORT_BYTES,) u8, is returned; best is chosen as
    without it, or with select_by_transfer by the largest transfer_inliers << 32
    | path.  transfer_mask: a sixth tensor, the transfer mask's words of best.
    three_view: all k selections also go through the three-view refinement
    (include/threeview/hc_pose_threeview.h; it implies fit_scale); the tuple is
    then (best, best_rank, refined, reports, scale reports, three-view reports
    (k * THREEVIEW_REPORT_BYTES,) u8), best is chosen by the final joint key, or
    with select_by_transfer by the final transfer_inliers << 32 | path.
    structure (which implies three_view): the 3D edgels of best, after the
    selection, from tangents (E, 6) f32; two more tensors follow, the records
    (E * EDGEL3D_BYTES,) u8 and the structure report."""
    what = "refine_topk"
    _refine_settings(iterations, min_inliers, what)
    _check_three_view(what, _check_structure(what, structure, tangents, min_sin_plane, max_sin3, three_view),
                      three_view_iterations, fit_scale)
    return _launch_refine_topk(what, candidates, _topk_count(candidates, what), (edgels, K), iterations, min_inliers,
                               stream, refined, fit_scale, transfer_mask, select_by_transfer, three_view,
                               three_view_iterations, structure, tangents, min_sin_plane, max_sin3)


def _refine_topk_dicts(best, best_rank, refined, reports, T, k, scale=None, words=None, three_view=None):
    sels = _selection_dicts(refined, T * k)
    reps = [refine_report_dict(r) for r in reports.cpu().numpy().reshape(T * k, REPORT_BYTES)]
    if scale is not None:
        for r, sc in zip(reps, _scale_report_dicts(scale, T * k)):
            r["scale"] = sc
    if three_view is not None:
        for r, tv in zip(reps, _three_view_report_dicts(three_view, T * k)):
            r["three_view"] = tv
    ranks = best_rank.cpu().numpy()
    out = [dict(best=b, best_rank=int(ranks[t]), refined=sels[t * k:(t + 1) * k], reports=reps[t * k:(t + 1) * k])
           for t, b in enumerate(_selection_dicts(best, T))]
    if words is not None:
        out[0]["transfer_mask"] = _mask_words(words)
    return out


def refine_topk(candidates, edgels: torch.Tensor, K: torch.Tensor, iterations: int = 10, min_inliers: int = 16,
                fit_scale: bool = False, transfer_mask: bool = False, select_by_transfer: bool = False,
                three_view: bool = False, three_view_iterations: int | None = None, structure: bool = False,
                tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Synchronous wrapper: (best dict, best_rank, [refined dict] * k, [report dict] * k).
    With fit_scale every report dict has a "scale" entry; with transfer_mask
    best's entry (reports[best_rank]["scale"]) also has "mask", the packed words.
    With three_view every report dict also has a "three_view" entry.  With
    structure (which implies three_view) two more values follow: best's
    structure report as a dict and its records."""
    out = launch_refine_topk(candidates, edgels, K, iterations, min_inliers, fit_scale=fit_scale,
                             transfer_mask=transfer_mask, select_by_transfer=select_by_transfer,
                             three_view=three_view, three_view_iterations=three_view_iterations, structure=structure,
                             tangents=tangents, min_sin_plane=min_sin_plane, max_sin3=max_sin3)
    torch.cuda.synchronize(edgels.device)
    d = _refine_topk_dicts(*out[:4], 1, _topk_count(candidates, "refine_topk"),
                           *_topk_extra(out, three_view or structure))[0]
    if "transfer_mask" in d and d["best_rank"] >= 0:
        d["reports"][d["best_rank"]]["scale"]["mask"] = d["transfer_mask"]
    if structure:
        srep = structure_report_dict(out[7])
        return d["best"], d["best_rank"], d["refined"], d["reports"], srep, structure_records(out[6], srep)
    return d["best"], d["best_rank"], d["refined"], d["reports"]


def launch_refine_topk_grouped(candidates, batch, k: int, iterations: int = 10, min_inliers: int = 16, stream=None,
                               refined: torch.Tensor | None = None, fit_scale: bool = False,
                               transfer_mask: bool = False, select_by_transfer: bool = False,
                               three_view: bool = False, three_view_iterations: int | None = None,
                               structure: bool = False, tangents: torch.Tensor | None = None,
                               min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Enqueue hc_trifocal_pose_refine_topk_grouped (no sync): candidates
    [t * k + r] refined on triplet t of batch (a multi.DeviceTripletBatch), one
    selection per triplet.  Returns (best (T * JOINT_SEL_BYTES,) u8, best_rank
    (T,) i32, refined, reports), and with fit_scale also the T * k scale reports
    (select_by_transfer as in launch_refine_topk; transfer_mask is refused);
    with three_view the scale reports and the T * k three-view reports; with
    structure (which implies three_view; tangents: the batch's own unless given)
    also the records of every triplet's best and the T structure reports."""
    _check_k(k, "refine_topk_grouped")
    return _launch_refine_topk("refine_topk_grouped", candidates, k, batch, iterations, min_inliers, stream, refined,
                               fit_scale, transfer_mask, select_by_transfer, three_view, three_view_iterations,
                               structure, tangents, min_sin_plane, max_sin3)


def refine_topk_grouped(candidates, batch, k: int, iterations: int = 10, min_inliers: int = 16, device=None,
                        fit_scale: bool = False, transfer_mask: bool = False, select_by_transfer: bool = False,
                        three_view: bool = False, three_view_iterations: int | None = None, structure: bool = False,
                        tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Synchronous wrapper: per triplet a dict(best, best_rank, refined, reports)
    of dicts.  batch: a multi.TripletBatch (copied to device, or to the
    candidates' device) or a multi.DeviceTripletBatch.  With fit_scale every
    report dict has a "scale" entry, with three_view also a "three_view" entry.
    With structure (which implies three_view) every triplet's dict also has
    "structure_report" and "structure", those of its best."""
    _check_k(k, "refine_topk_grouped")
    _refine_settings(iterations, min_inliers, "refine_topk_grouped")
    three_view = _check_structure("refine_topk_grouped", structure, tangents, min_sin_plane, max_sin3, three_view)
    _check_scale_flags("refine_topk_grouped", _check_three_view("refine_topk_grouped", three_view,
                                                                 three_view_iterations, fit_scale),
                       transfer_mask, select_by_transfer, mask_allowed=False)
    if not hasattr(batch, "groups"):
        if device is None:
            device = candidates.device if isinstance(candidates, torch.Tensor) else "cuda:0"
        batch = batch.to(device)
    out = launch_refine_topk_grouped(candidates, batch, k, iterations, min_inliers, fit_scale=fit_scale,
                                     transfer_mask=transfer_mask, select_by_transfer=select_by_transfer,
                                     three_view=three_view, three_view_iterations=three_view_iterations,
                                     structure=structure, tangents=tangents, min_sin_plane=min_sin_plane,
                                     max_sin3=max_sin3)
    torch.cuda.synchronize(batch.device)
    res = _refine_topk_dicts(*out[:4], batch.num_groups, k, *_topk_extra(out, three_view))
    if structure:
        sreps = _structure_report_dicts(out[7], batch.num_groups)
        for d, r, rec in zip(res, sreps, _group_records(out[6], sreps, batch)):
            d["structure_report"], d["structure"] = r, rec
    return res


def merge_topk(parts: list, path_offsets: list, k: int) -> list:
    """hc_pose_merge_topk: the top-k lists of several launches / GPUs (each a
    list of k dicts / structs, or the raw bytes of k selections) with their first
    batch ids -> the k best of all, with global batch ids."""
    k = _check_k(k, "merge_topk")
    n = len(parts)
    if len(path_offsets) != n:
        raise _abi.HCError(f"merge_topk: {len(path_offsets)} offsets for {n} parts")
    arr = (_abi.hcTrifocalSelection * max(1, n * k))()
    for i, part in enumerate(parts):
        if isinstance(part, (torch.Tensor, np.ndarray)):
            raw = part.cpu().numpy() if isinstance(part, torch.Tensor) else part
            raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
            part = [raw[j * JOINT_SEL_BYTES:(j + 1) * JOINT_SEL_BYTES] for j in range(raw.size // JOINT_SEL_BYTES)]
        if len(part) != k:
            raise _abi.HCError(f"merge_topk: part {i} has {len(part)} selections, not {k}")
        for j, p in enumerate(part):
            arr[i * k + j] = joint_selection_from_dict(p) if isinstance(p, dict) else joint_selection_struct(p)
    offs = np.ascontiguousarray(path_offsets if n else [0], np.int32)
    out = (_abi.hcTrifocalSelection * k)()
    _abi.lib().hc_pose_merge_topk(n, k, C.cast(arr, C.c_void_p), _abi.ptr(offs), C.cast(out, C.c_void_p))
    return [joint_selection_dict(s) for s in out]


def select_refined(tracks: torch.Tensor, converge: torch.Tensor, edgels: torch.Tensor, K: torch.Tensor, k: int = 8,
                   iterations: int = 10, min_inliers: int = 16, stream=None, fit_scale: bool = False,
                   transfer_mask: bool = False, select_by_transfer: bool = False, three_view: bool = False,
                   three_view_iterations: int | None = None, structure: bool = False,
                   tangents: torch.Tensor | None = None, min_sin_plane: float = 0.05, max_sin3: float = 0.05):
    """Joint pose support, the k best candidates, their refinement and the
    selection among the refined ones, enqueued on one stream with a single
    synchronisation at the end.  Returns (best dict, info); info: joint (the
    joint call's winner, = candidate 0), best_rank, candidates and refined
    ([dict] * k), refined_inliers ([int] * k, -1 for a "none" rank) and reports.
    With fit_scale every report has a "scale" entry and info has scale, best's
    own (None without a best; with transfer_mask it holds "mask");
    select_by_transfer as in launch_refine_topk.  With three_view (which
    implies fit_scale) every report also has a "three_view" entry and info has
    three_view, best's own (None without a best); a transfer mask is refused.
    With structure (which implies three_view) info has structure_report, the
    structure report of best as a dict, and structure, its records."""
    what = "select_refined"
    k = _check_k(k, what)
    _refine_settings(iterations, min_inliers, what)
    three_view = _check_structure(what, structure, tangents, min_sin_plane, max_sin3, three_view)
    fit_scale = _check_three_view(what, three_view, three_view_iterations, fit_scale)
    _check_scale_flags(what, fit_scale, transfer_mask, select_by_transfer)
    if three_view and transfer_mask:
        raise _abi.HCError(f"{what}: with three_view the transfer mask is written by refine_joint only")
    dev = tracks.device
    n = converge.numel()
    inl = torch.empty((n, 3), dtype=torch.int32, device=dev)
    sel = torch.empty(JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    launch_pose_support_joint(tracks, converge, edgels, K, inl, sel, stream)
    cand = launch_topk_joint(tracks, inl, k, stream=stream)
    out = launch_refine_topk(cand, edgels, K, iterations, min_inliers, stream, fit_scale=fit_scale,
                             transfer_mask=transfer_mask, select_by_transfer=select_by_transfer,
                             three_view=three_view, three_view_iterations=three_view_iterations, structure=structure,
                             tangents=tangents, min_sin_plane=min_sin_plane, max_sin3=max_sin3)
    stream.synchronize()
    d = _refine_topk_dicts(*out[:4], 1, k, *_topk_extra(out, three_view))[0]
    info = dict(joint=joint_selection_dict(joint_selection_struct(sel)), best_rank=d["best_rank"],
                candidates=_selection_dicts(cand, k), refined=d["refined"],
                refined_inliers=[r["inliers"] for r in d["refined"]], reports=d["reports"])
    if fit_scale:
        info["scale"] = None
        if d["best_rank"] >= 0:
            info["scale"] = dict(d["reports"][d["best_rank"]]["scale"])
            if "transfer_mask" in d:
                info["scale"]["mask"] = d["transfer_mask"]
    if three_view:
        info["three_view"] = dict(d["reports"][d["best_rank"]]["three_view"]) if d["best_rank"] >= 0 else None
    if structure:
        info["structure_report"] = structure_report_dict(out[7])
        info["structure"] = structure_records(out[6], info["structure_report"])
    return d["best"], info


def residuals(data: RansacData, sel: dict):
    """Measure_Relative_Pose_Error: ([rot21, rot31, transl21, transl31], success)."""
    out = np.zeros(4, np.float32)
    a = [np.ascontiguousarray(v, np.float32) for v in (data.pose21, data.pose31, sel["R21"], sel["t21"],
                                                        sel["R31"], sel["t31"])]
    ok = _abi.lib().hc_pose_residuals(*[_abi.ptr(v) for v in a], _abi.ptr(out))
    return out, bool(ok)


def success_clamped(data: RansacData, sel: dict, out: np.ndarray) -> bool:
    """The GT verdict with the rotation residual's acos argument clamped to
    [-1, 1].  The reference (Evaluations.cpp:360-374) does not clamp: an exact
    rotation whose float trace rounds above 3 gives acos(> 1) = NaN, and the
    pose counts as a failure.  Reported beside the reference verdict, never
    instead of it."""
    rot = []
    for gt, R in ((data.pose21, sel["R21"]), (data.pose31, sel["R31"])):
        G = np.asarray(gt, np.float64)[:9].reshape(3, 3)
        M = G.T @ np.asarray(R, np.float64).reshape(3, 3)
        rot.append(float(np.arccos(np.clip(0.5 * (np.trace(M) - 1.0), -1.0, 1.0))))
    return bool(rot[0] < 0.1 and rot[1] < 0.1 and float(out[2]) < 0.1 and float(out[3]) < 0.1)
