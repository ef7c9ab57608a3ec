"""ctypes binding of the C-ABI in include/*.h.

The native library (lib/libhc_trifocal.so, HIP for gfx950) is the product: this
module only marshals pointers.  It raises if the library is missing -- there is
no CPU fallback anywhere in the product path.

The boundary is described once: the ctypes mirrors of the argument structs and
SIGNATURES, one (name, restype, argtypes, optional) entry per declared function.
lib() binds the table, DECLARED_SYMBOLS is its names, and tests/test_abi_host.py
holds both against the headers (layouts through the C compiler, signatures
against the prototypes).  The headers in directories of their own
(include/p2c, include/refine, include/topk, include/adaptive) have tables of their own,
P2C_SIGNATURES, REFINE_SIGNATURES, TOPK_SIGNATURES and ADAPTIVE_SIGNATURES, checked the same way
(include/scale, include/threeview and include/structure declare structs only: the scale fit, the three-view refinement and the reconstruction are modes of the refine calls).  Callers go through two helpers: ptr(x), the c_void_p
of a tensor, array or stream, and call(name, *args), which raises HCError on a
status other than HC_SUCCESS.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# HC_TRIFOCAL_LIB: an alternative build of the same library (A/B experiments,
# scripts/build_variant.sh)
LIB_PATH = os.environ.get("HC_TRIFOCAL_LIB") or os.path.join(PKG_DIR, "lib", "libhc_trifocal.so")

# include/hc_trifocal.h HC_TRIFOCAL_ABI_VERSION: the struct layouts below
ABI_VERSION = 2

NUM_VARS, NUM_PARAMS, NUM_TRACKS = 30, 33, 312
NPP = NUM_PARAMS + 1
UNIFIED_INDEX_SIZE = 38880

HC_STATUS = {0: "HC_SUCCESS", 1: "HC_ERROR_INVALID_VALUE", 2: "HC_ERROR_WORKSPACE", 3: "HC_ERROR_LAUNCH",
             4: "HC_ERROR_DEVICE", 5: "HC_ERROR_TABLE"}


class HCError(RuntimeError):
    pass


class hcTrackSettings(C.Structure):
    _fields_ = [("max_steps", C.c_int), ("max_corrections", C.c_int), ("delta_t_inc_steps", C.c_int)]


class hcTrackArgs(C.Structure):
    _fields_ = [("sub_ransac_iters", C.c_int),
                ("settings", hcTrackSettings),
                ("start_sols", C.c_void_p),
                ("start_sols_array", C.c_void_p),
                ("tracks", C.c_void_p),
                ("track_array", C.c_void_p),
                ("start_params", C.c_void_p),
                ("target_params", C.c_void_p),
                ("diff_params", C.c_void_p),
                ("unified_index", C.c_void_p),
                ("converge", C.c_void_p),
                ("infinity", C.c_void_p),
                ("stats", C.c_void_p)]


class hcPoseSelection(C.Structure):
    """include/hc_pose.h"""
    _fields_ = [("num_candidates", C.c_int32), ("path21", C.c_int32), ("inliers21", C.c_int32),
                ("path31", C.c_int32), ("inliers31", C.c_int32), ("pad", C.c_int32),
                ("key21", C.c_uint64), ("key31", C.c_uint64),
                ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("R31", C.c_float * 9), ("t31", C.c_float * 3)]


POSE_SELECTION_BYTES = C.sizeof(hcPoseSelection)


class hcTrifocalSelection(C.Structure):
    """include/hc_pose.h: one hypothesis for both views (joint selection)"""
    _fields_ = [("num_candidates", C.c_int32), ("path", C.c_int32), ("inliers", C.c_int32),
                ("inliers21", C.c_int32), ("inliers31", C.c_int32), ("pad", C.c_int32),
                ("key", C.c_uint64),
                ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("R31", C.c_float * 9), ("t31", C.c_float * 3),
                ("scale31", C.c_float), ("pad2", C.c_float)]


TRIFOCAL_SELECTION_BYTES = C.sizeof(hcTrifocalSelection)   # 136
HC_POSE_REFERENCE_QUIRKS = 1


class hcAbortArgs(C.Structure):
    _fields_ = [("num_triplet_edgels", C.c_int),
                ("triplet_edge_locations", C.c_void_p),
                ("intrinsic_matrix", C.c_void_p),
                ("found_trifocal_sols", C.c_void_p),
                ("trifocal_sols_batch_index", C.c_void_p),
                ("inflight_stop", C.c_int),
                ("peer_found", C.c_void_p)]


class hcTripletGroup(C.Structure):
    """One image triplet's scene data (device pointers): 24 bytes."""
    _fields_ = [("locations", C.c_void_p),
                ("K", C.c_void_p),
                ("num_edgels", C.c_int32),
                ("pad", C.c_int32)]


TRIPLET_GROUP_BYTES = C.sizeof(hcTripletGroup)


class hcGroupedAbortArgs(C.Structure):
    _fields_ = [("num_groups", C.c_int),
                ("groups", C.c_void_p),
                ("sample_group", C.c_void_p),
                ("group_found", C.c_void_p),
                ("trifocal_sols_batch_index", C.c_void_p),
                ("group_found_ticks", C.c_void_p),
                ("inflight_stop", C.c_int)]


class hcJointGate(C.Structure):
    """The stop rule of hc_trifocal_2op1p_30x30_track_abort_gated: 16 bytes."""
    _fields_ = [("min_joint_ratio", C.c_float),
                ("pad", C.c_int32),
                ("joint_inliers", C.c_void_p)]


HC_GATE_ADAPTIVE = 0x41445031   # include/adaptive/hc_trifocal_adaptive.h: hcJointGate::pad of an hcAdaptiveGate


class hcAdaptiveGate(C.Structure):
    """include/adaptive/hc_trifocal_adaptive.h: the gate of the gated launch's
    adaptive mode, 48 bytes; its address is passed as the hcJointGate's."""
    _fields_ = [("head", hcJointGate),
                ("need", C.c_void_p),
                ("need_offset", C.c_void_p),
                ("sample_ordinal", C.c_void_p),
                ("group_limit", C.c_void_p)]


class hcP2cArgs(C.Structure):
    """include/p2c/hc_trifocal_p2c.h: the P2C launch's own argument block, 32 bytes."""
    _fields_ = [("hx_index", C.c_void_p),
                ("ht_index", C.c_void_p),
                ("coeffs_hx", C.c_void_p),
                ("coeffs_ht", C.c_void_p)]


class hcIpcHandle(C.Structure):
    _fields_ = [("reserved", C.c_ubyte * 64)]


HC_REFINE_MAX_ITERATIONS = 32
HC_REFINE_NONE, HC_REFINE_TOO_FEW, HC_REFINE_SINGULAR = 1, 2, 4


class hcRefineSettings(C.Structure):
    """include/refine/hc_pose_refine.h: 16 bytes; 0 selects a default (10 iterations, 16 inliers)"""
    _fields_ = [("iterations", C.c_int32), ("min_inliers", C.c_int32), ("pad", C.c_int32 * 2)]


class hcRefineReport(C.Structure):
    """include/refine/hc_pose_refine.h: what one refinement did, 176 bytes"""
    _fields_ = [("status", C.c_int32), ("iterations_run", C.c_int32), ("best_iteration", C.c_int32),
                ("joint_history", C.c_int32 * (HC_REFINE_MAX_ITERATIONS + 1)),
                ("rms_px_in", C.c_double * 2), ("rms_px_out", C.c_double * 2)]


REFINE_REPORT_BYTES = C.sizeof(hcRefineReport)   # 176

# include/scale/hc_pose_scale.h: the scale fit, a mode of the refine calls (no
# function of its own; its structs are held against the header by
# tests/test_scale31_host.py)
HC_REFINE_SCALE31 = 0x53433331   # hcRefineSettings::pad[0] of an hcRefineScaleSettings
HC_SCALE_ONLY, HC_SCALE_SELECT_BY_TRANSFER = 1, 2   # pad[1]: mode bits
HC_SCALE_NONE, HC_SCALE_NO_VOTER = 1, 2              # hcScaleReport::status bits


class hcScaleReport(C.Structure):
    """include/scale/hc_pose_scale.h: what one scale fit did, 40 bytes"""
    _fields_ = [("status", C.c_int32), ("num_voters", C.c_int32), ("voter", C.c_int32),
                ("transfer_inliers", C.c_int32), ("tested", C.c_int32), ("joint", C.c_int32),
                ("scale_in", C.c_float), ("scale31", C.c_float), ("key", C.c_uint64)]


class hcRefineScaleSettings(C.Structure):
    """include/scale/hc_pose_scale.h: the settings of the scale mode, 32 bytes;
    its address is passed as the hcRefineSettings'."""
    _fields_ = [("head", hcRefineSettings), ("reports", C.c_void_p), ("transfer_mask", C.c_void_p)]


SCALE_REPORT_BYTES = C.sizeof(hcScaleReport)   # 40

# include/threeview/hc_pose_threeview.h: the three-view refinement, a further mode
# of the refine calls (no function of its own; its structs and the table below
# are held against the header by tests/test_threeview_host.py)
HC_REFINE_THREEVIEW = 0x54563331          # hcRefineSettings::pad[0] of an hcRefineThreeViewSettings
HC_THREEVIEW_SELECT_BY_TRANSFER = 2       # pad[1]: mode bits
HC_THREEVIEW_NONE, HC_THREEVIEW_TOO_FEW, HC_THREEVIEW_SINGULAR, HC_THREEVIEW_SKIPPED = 1, 2, 4, 8   # status bits
THREEVIEW_CONSTANTS = {"HC_REFINE_THREEVIEW": HC_REFINE_THREEVIEW,
                       "HC_THREEVIEW_SELECT_BY_TRANSFER": HC_THREEVIEW_SELECT_BY_TRANSFER,
                       "HC_THREEVIEW_NONE": HC_THREEVIEW_NONE, "HC_THREEVIEW_TOO_FEW": HC_THREEVIEW_TOO_FEW,
                       "HC_THREEVIEW_SINGULAR": HC_THREEVIEW_SINGULAR, "HC_THREEVIEW_SKIPPED": HC_THREEVIEW_SKIPPED}


class hcThreeViewReport(C.Structure):
    """include/threeview/hc_pose_threeview.h: what one three-view refinement did, 328 bytes"""
    _fields_ = [("status", C.c_int32), ("iterations_run", C.c_int32), ("best_iteration", C.c_int32),
                ("transfer_history", C.c_int32 * (HC_REFINE_MAX_ITERATIONS + 1)),
                ("joint_history", C.c_int32 * (HC_REFINE_MAX_ITERATIONS + 1)),
                ("fit_set", C.c_int32), ("transfer_inliers", C.c_int32),
                ("scale_in", C.c_float), ("scale_out", C.c_float), ("pad", C.c_int32),
                ("rms_px_in", C.c_double * 2), ("rms_px_out", C.c_double * 2)]


class hcRefineThreeViewSettings(C.Structure):
    """include/threeview/hc_pose_threeview.h: the settings of the three-view mode,
    48 bytes; its address is passed as the hcRefineSettings'."""
    _fields_ = [("head", hcRefineSettings), ("scale_reports", C.c_void_p), ("reports", C.c_void_p),
                ("transfer_mask", C.c_void_p), ("iterations3", C.c_int32), ("pad", C.c_int32)]


THREEVIEW_REPORT_BYTES = C.sizeof(hcThreeViewReport)   # 328

# include/structure/hc_pose_structure.h: the reconstruction of the 3D edgels, a
# further mode of the refine calls (no function of its own; its structs and the
# table below are held against the header by tests/test_structure_host.py)
HC_REFINE_STRUCTURE = 0x53543344          # hcRefineSettings::pad[0] of an hcRefineStructureSettings
HC_STRUCTURE_ONLY = 1                     # pad[1]: mode bit (bit 2 stays HC_THREEVIEW_SELECT_BY_TRANSFER)
HC_EDGEL3D_TANGENT, HC_EDGEL3D_ORIENTED = 1, 2   # hcEdgel3D::flags
HC_STRUCTURE_NONE = 1                     # hcStructureReport::status
STRUCTURE_CONSTANTS = {"HC_REFINE_STRUCTURE": HC_REFINE_STRUCTURE, "HC_STRUCTURE_ONLY": HC_STRUCTURE_ONLY,
                       "HC_EDGEL3D_TANGENT": HC_EDGEL3D_TANGENT, "HC_EDGEL3D_ORIENTED": HC_EDGEL3D_ORIENTED,
                       "HC_STRUCTURE_NONE": HC_STRUCTURE_NONE}


class hcEdgel3D(C.Structure):
    """include/structure/hc_pose_structure.h: one reconstructed edgel, 48 bytes"""
    _fields_ = [("X", C.c_float * 3), ("T", C.c_float * 3), ("err3_px", C.c_float), ("sin_plane", C.c_float),
                ("sin3", C.c_float), ("edgel", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32)]


class hcStructureReport(C.Structure):
    """include/structure/hc_pose_structure.h: what one reconstruction did, 32 bytes"""
    _fields_ = [("status", C.c_int32), ("count", C.c_int32), ("tangents", C.c_int32), ("oriented", C.c_int32),
                ("scale31", C.c_float), ("pad", C.c_int32 * 3)]


class hcRefineStructureSettings(C.Structure):
    """include/structure/hc_pose_structure.h: the settings of the structure mode,
    88 bytes; its address is passed as the hcRefineSettings'."""
    _fields_ = [("tv", hcRefineThreeViewSettings), ("tangents", C.c_void_p), ("edgel_offsets", C.c_void_p),
                ("edgels3d", C.c_void_p), ("reports", C.c_void_p), ("min_sin_plane", C.c_float),
                ("max_sin3", C.c_float)]


EDGEL3D_BYTES = C.sizeof(hcEdgel3D)                    # 48
STRUCTURE_REPORT_BYTES = C.sizeof(hcStructureReport)   # 32
# hcEdgel3D as a numpy record
EDGEL3D_DTYPE = np.dtype([("X", "<f4", (3,)), ("T", "<f4", (3,)), ("err3_px", "<f4"), ("sin_plane", "<f4"),
                          ("sin3", "<f4"), ("edgel", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert EDGEL3D_DTYPE.itemsize == EDGEL3D_BYTES


# One entry per function of include/*.h: restype and argtypes as the prototype
# reads (None for void; c_void_p for device and host buffers and for hcStream,
# POINTER(struct) for the argument structs, c_char_p for paths).  optional: a
# build from before the symbol existed, loaded through HC_TRIFOCAL_LIB for an
# A/B run, may lack it; it is then left unbound and call() says so.  The product
# library exports all of them (tests/test_abi_host.py, which also checks every
# entry against its prototype).
Sig = namedtuple("Sig", "name restype argtypes optional", defaults=(False,))

_i, _u, _z, _p, _s, _ST = C.c_int, C.c_uint, C.c_size_t, C.c_void_p, C.c_char_p, C.c_int   # _ST: hcStatus
_TA = C.POINTER(hcTrackArgs)
_GA = C.POINTER(hcGroupedAbortArgs)
_WS = (_p, _z, _p)                                           # workspace, workspace_bytes, stream
_SUPPORT = (_i, _p, _p, _i, _p, _p, _i, _p, _p, _p)          # the four pose-support calls

SIGNATURES = (
    # include/hc_trifocal.h
    Sig("hc_trifocal_workspace_size", _z, ()),
    Sig("hc_trifocal_workspace_size_for", _z, (_i,)),
    Sig("hc_trifocal_workspace_size_for_steps", _z, (_i, _i)),
    Sig("hc_trifocal_2op1p_30x30_track", _ST, (_TA, *_WS)),
    Sig("hc_trifocal_2op1p_30x30_track_abort", _ST, (_TA, C.POINTER(hcAbortArgs), *_WS)),
    Sig("hc_trifocal_2op1p_30x30_track_abort_grouped", _ST, (_TA, _GA, *_WS), True),
    Sig("hc_trifocal_2op1p_30x30_track_abort_gated", _ST, (_TA, _GA, C.POINTER(hcJointGate), *_WS), True),
    Sig("hc_shared_flag_create", _ST, (C.POINTER(_p), C.POINTER(hcIpcHandle)), True),
    Sig("hc_shared_flag_memory_kind", _i, (_p,), True),
    Sig("hc_shared_flag_open", _ST, (C.POINTER(hcIpcHandle), C.POINTER(_p)), True),
    Sig("hc_shared_flag_reset", _ST, (_p, _p), True),
    Sig("hc_shared_flag_close", _ST, (_p, _i), True),
    Sig("hc_trifocal_2op1p_30x30_track_ph_codeopt", _ST, (_TA, *_WS)),
    Sig("hc_trifocal_2op1p_30x30_track_ph", _ST, (_TA, *_WS)),
    Sig("hc_trifocal_workspace_status", _ST, (_p,)),
    Sig("hc_trifocal_read_timings", _ST, (_p, C.POINTER(C.c_double))),
    Sig("hc_trifocal_read_timestamps", _ST, (_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_double))),
    Sig("hc_cgesv_30x30_batched", _ST, (_i, _p, _p, _p, _p)),
    Sig("hc_trifocal_eval_batched", _ST, (_i, _p, _p, _p, _p, _p, _p, _p, *_WS)),
    Sig("hc_last_error_string", _s, ()),
    Sig("hc_trifocal_version", _s, ()),
    Sig("hc_trifocal_abi_version", _i, ()),
    # include/hc_trifocal_testing.h (test hooks)
    Sig("hc_trifocal_set_ring_test", None, (_i,)),
    Sig("hc_trifocal_set_small_launch", None, (_i,), True),
    Sig("hc_trifocal_set_retry_reuse", None, (_i,), True),
    Sig("hc_trifocal_ring_check_test", _ST, (_p, _z, _u, _u, _u, _p), True),
    Sig("hc_lu_struct_pattern", _u, (_i,), True),
    Sig("hc_lu_group_class", _i, (_i, _i), True),
    Sig("hc_lu_candidates", _u, (_i,), True),
    Sig("hc_lu_search_span", _i, (_i,), True),
    # include/hc_pose.h
    Sig("hc_trifocal_pose_support", _ST, _SUPPORT),
    Sig("hc_trifocal_pose_support_grouped", _ST, _SUPPORT, True),
    Sig("hc_pose_merge", None, (_i, _p, _p, _i, C.POINTER(hcPoseSelection))),
    Sig("hc_trifocal_pose_support_joint", _ST, _SUPPORT),
    Sig("hc_trifocal_pose_support_joint_grouped", _ST, _SUPPORT),
    Sig("hc_trifocal_pose_inlier_mask", _ST, (_p, _i, _p, _p, _p, _p)),
    Sig("hc_pose_merge_joint", None, (_i, _p, _p, C.POINTER(hcTrifocalSelection))),
    Sig("hc_pose_residuals", _i, (_p,) * 7),
    # include/hc_host.h
    Sig("hc_read_start_sols", _i, (_s, _p)),
    Sig("hc_read_start_params", _i, (_s, _p)),
    Sig("hc_read_int_table", _i, (_s, _p, _i)),
    Sig("hc_read_float_table", _i, (_s, _p, _i)),
    Sig("hc_count_triplet_edgels", _i, (_s,)),
    Sig("hc_read_triplet_edgels", _i, (_s, _p, _p, _i)),
    Sig("hc_split_samples", None, (_i, _i, _p)),
    Sig("hc_prepare_target_params", None, (_u, _i, _p, _p, _p, _i, _p, _p, _p, _p)),
    Sig("hc_count_solutions", None, (_i, _p, _p, _p, _p)),
    Sig("hc_write_converged_sols", _i, (_s, _i, _p, _p)),
    Sig("hc_add_pixel_noise", None, (_i, _p, _p, C.c_double, C.c_uint64, _p)),
    Sig("hc_write_triplet_edgels", _i, (_s, _i, _p, _p)),
)
DECLARED_SYMBOLS = tuple(s.name for s in SIGNATURES)

# include/p2c/hc_trifocal_p2c.h, the P2C mode's header beside include/*.h: a table
# of its own, bound by lib() like SIGNATURES and held against its header the same
# way (tests/test_p2c_host.py)
P2C_SIGNATURES = (
    Sig("hc_trifocal_2op1p_30x30_track_p2c", _ST, (_TA, C.POINTER(hcP2cArgs), *_WS), True),
    Sig("hc_trifocal_p2c_eval_batched", _ST, (_i, _p, _p, _p, _p, _p, _p, _p, _p, _p, *_WS), True),
    Sig("hc_p2c_coefficients", _ST, (_i, _p, _p, _p, _p, _p), True),
)
P2C_DECLARED_SYMBOLS = tuple(s.name for s in P2C_SIGNATURES)

# include/refine/hc_pose_refine.h, the pose refinement's header beside
# include/hc_pose.h: its table, bound and checked the same way
# (tests/test_refine_host.py)
_RS = C.POINTER(hcRefineSettings)
REFINE_SIGNATURES = (
    Sig("hc_trifocal_pose_refine", _ST, (_p, _i, _p, _p, _RS, _p, _p, _p), True),
    Sig("hc_trifocal_pose_refine_grouped", _ST, (_i, _p, _p, _RS, _p, _p, _p), True),
)
REFINE_DECLARED_SYMBOLS = tuple(s.name for s in REFINE_SIGNATURES)

# include/topk/hc_pose_topk.h, the top-k candidates' header beside the refinement's:
# its table, bound and checked the same way (tests/test_topk_host.py)
HC_TOPK_MAX = 32
TOPK_SIGNATURES = (
    Sig("hc_trifocal_pose_topk_joint", _ST, (_i, _p, _p, _i, _p, _p), True),
    Sig("hc_trifocal_pose_topk_joint_grouped", _ST, (_i, _p, _p, _i, _p, _i, _p, _p), True),
    Sig("hc_trifocal_pose_refine_topk", _ST, (_i, _p, _i, _p, _p, _RS, _p, _p, _p, _p, _p), True),
    Sig("hc_trifocal_pose_refine_topk_grouped", _ST, (_i, _p, _i, _p, _RS, _p, _p, _p, _p, _p), True),
    Sig("hc_pose_merge_topk", None, (_i, _i, _p, _p, _p), True),
)
TOPK_DECLARED_SYMBOLS = tuple(s.name for s in TOPK_SIGNATURES)

# include/lu/hc_lu_testing.h, the fused LU levels' test hooks beside
# include/hc_trifocal_testing.h: its table, bound and checked the same way
# (tests/test_lu_levels.py)
LU_SIGNATURES = (
    Sig("hc_lu_step_level", _i, (_i,), True),
    Sig("hc_cgesv_30x30_struct_batched", _ST, (_i, _p, _p, _p, _p), True),
    Sig("hc_cgesv_30x30_variant_batched", _ST, (_i, _i, _p, _p, _p, _p), True),
)
# hcLuVariant, in the header's order: the instantiations of the tracker's sparse
# solve by the kernels that run them (odd: the structure-agnostic twins)
LU_VARIANTS = ("throughput", "throughput_twin", "abort", "abort_twin", "small", "small_twin", "archived",
               "archived_twin")
LU_DECLARED_SYMBOLS = tuple(s.name for s in LU_SIGNATURES)

# include/lu/hc_lu_rowtable_testing.h, the fused levels' row records beside the
# LU's other test hooks (tests/test_lu_rowtable_host.py); hcLuRowField in the
# header's order
LU_ROWTABLE_SIGNATURES = (
    Sig("hc_lu_row_field", _i, (_i, _i, _i), True),
)
LU_ROW_FIELDS = ("member", "bound", "window", "partner", "place", "chain")

# include/lu/hc_lu_compact_testing.h, the fused solve's compact row beside the
# row records (tests/test_lu_compact_host.py); neither takes a stream
LU_COMPACT_SIGNATURES = (
    Sig("hc_lu_compact_column", _i, (_i, _i), True),
    Sig("hc_trifocal_compact_rows_batched", _ST, (_i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.c_size_t), True),
)
LU_COMPACT_WIDTH = 16

# include/eval/hc_eval_testing.h, the test hook of the tracking kernels' evaluations
# beside the LU's: its table, bound and checked the same way
# (tests/test_eval_cases_host.py)
EVAL_SIGNATURES = (
    Sig("hc_trifocal_eval_variant_batched", _ST, (_i, _u, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, *_WS), True),
)
# hcEvalVariant, in the header's order: the tables the evaluations read
EVAL_VARIANTS = ("packed", "abs")
HC_EVAL_REDO = 1
EVAL_DECLARED_SYMBOLS = tuple(s.name for s in EVAL_SIGNATURES)

# include/adaptive/hc_trifocal_adaptive.h, the adaptive sample limit's header beside
# include/hc_trifocal.h: no launch of its own (a mode of the gated one), one host
# function; its table, bound and checked the same way (tests/test_adaptive_host.py)
ADAPTIVE_SIGNATURES = (
    Sig("hc_ransac_need_table", _ST, (_i, C.c_double, _i, _i, _p), True),
)
ADAPTIVE_DECLARED_SYMBOLS = tuple(s.name for s in ADAPTIVE_SIGNATURES)

_lib = None


def lib() -> C.CDLL:
    """Load the native library (raises HCError if it has not been built) and
    bind every entry of SIGNATURES it exports."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HCError(f"native library missing: {LIB_PATH} (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        # torch is the process' HIP runtime owner (device memory, streams):
        # load it first so libhc_trifocal.so binds to the same libamdhip64.so.7
        # instead of pulling a second HIP/HSA runtime from /opt/rocm.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for s in SIGNATURES + P2C_SIGNATURES + REFINE_SIGNATURES + TOPK_SIGNATURES + LU_SIGNATURES + \
                LU_ROWTABLE_SIGNATURES + LU_COMPACT_SIGNATURES + EVAL_SIGNATURES + ADAPTIVE_SIGNATURES:
            fn = getattr(L, s.name, None)
            if fn is None:
                if s.optional:
                    continue
                raise HCError(f"{LIB_PATH} does not export {s.name}")
            fn.restype, fn.argtypes = s.restype, list(s.argtypes)
        if L.hc_trifocal_abi_version() != ABI_VERSION:
            raise HCError(f"{LIB_PATH}: ABI {L.hc_trifocal_abi_version()}, this binding expects {ABI_VERSION}")
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        detail = lib().hc_last_error_string().decode(errors="replace")
        raise HCError(f"{what} failed: {HC_STATUS.get(status, status)} ({detail})")


def call(name: str, *args) -> None:
    """Call the hcStatus-returning entry point `name`; a status other than
    HC_SUCCESS raises HCError, and so does a symbol the loaded build lacks."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise HCError(f"{LIB_PATH} does not export {name}")
    check(fn(*args), name)


def ptr(x):
    """The c_void_p of a buffer or stream: a torch tensor's device (or host)
    address, a numpy array's (the pointer keeps the array alive), a torch
    stream's hipStream_t; None is NULL."""
    if x is None:
        return C.c_void_p()
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if hasattr(x, "cuda_stream"):
        return C.c_void_p(x.cuda_stream)
    return x.ctypes.data_as(C.c_void_p)


def _fatbin_digest(path: str) -> str | None:
    """sha256 of the .hip_fatbin section of an ELF shared library: the gfx950
    code objects of every kernel, independent of the host code around them."""
    import hashlib
    import struct
    with open(path, "rb") as fh:
        elf = fh.read()
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        return None
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    def sec(i):
        name, _typ, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        return name, off, size
    _, stroff, _ = sec(shstrndx)
    for i in range(shnum):
        name, off, size = sec(i)
        end = elf.index(b"\0", stroff + name)
        if elf[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(elf[off:off + size]).hexdigest()
    return None


def build_id(path: str | None = None) -> str:
    """Identifies the kernels a profile or bench line measured: the library's
    version tag and the first 12 hex digits of the sha256 of its device code
    (.hip_fatbin).  Profiles under profiles/ carry it and bench.py takes its
    PMC / LU-work sources only from profiles of the loaded build."""
    import re
    path = path or LIB_PATH
    with open(path, "rb") as fh:
        m = re.search(rb"hc_trifocal gfx950 (v[0-9.]+)", fh.read())
    ver = m.group(1).decode() if m else "v?"
    d = _fatbin_digest(path)
    return f"{ver}+{d[:12] if d else 'nofatbin'}"


PRODUCT_LIB_PATH = os.path.join(PKG_DIR, "lib", "libhc_trifocal.so")
