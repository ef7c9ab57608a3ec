"""CPU tests of the gated abort launch's host side
(hc_trifocal_2op1p_30x30_track_abort_gated): the export, the hcJointGate
layout, the argument checks made before any device work, and the Python
wrapper's gate validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    assert "hc_trifocal_2op1p_30x30_track_abort_gated" in _abi.DECLARED_SYMBOLS
    L = _abi.lib()
    assert hasattr(L, "hc_trifocal_2op1p_30x30_track_abort_gated")
    hdr = open(os.path.join(ROOT, "include", "hc_trifocal.h")).read()
    assert "hc_trifocal_2op1p_30x30_track_abort_gated(" in hdr


def test_joint_gate_layout_and_abi_version():
    """sizeof(hcJointGate) of the header, compiled by the host compiler's rules
    (float, int32, pointer: 16 bytes), equals the ctypes struct; additive, so
    the ABI version stays 2."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    g = _abi.hcJointGate
    assert C.sizeof(g) == 16
    assert (g.min_joint_ratio.offset, g.pad.offset, g.joint_inliers.offset) == (0, 4, 8)
    hdr = open(os.path.join(ROOT, "include", "hc_trifocal.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} hcJointGate;", hdr)
    assert m, "hcJointGate not declared"
    fields = re.findall(r"^\s*(float|int32_t)\s+(\*?)(\w+);", m.group(1), re.M)
    assert fields == [("float", "", "min_joint_ratio"), ("int32_t", "", "pad"), ("int32_t", "*", "joint_inliers")]
    assert "#define HC_TRIFOCAL_ABI_VERSION 2" in hdr
    assert _abi.lib().hc_trifocal_abi_version() == _abi.ABI_VERSION == 2


def test_joint_gate_sizeof_by_the_c_compiler(tmp_path):
    """The header through a C compiler (whichever the machine has; the build
    needs one): sizeof and offsetof of hcJointGate equal the ctypes struct's."""
    import shutil
    import subprocess

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    src = tmp_path / "gate.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hc_trifocal.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(hcJointGate), '
                   'offsetof(hcJointGate, min_joint_ratio), offsetof(hcJointGate, pad), '
                   'offsetof(hcJointGate, joint_inliers)); return 0; }\n')
    exe = tmp_path / "gate"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.split()
    g = _abi.hcJointGate
    assert [int(v) for v in out] == [C.sizeof(g), g.min_joint_ratio.offset, g.pad.offset, g.joint_inliers.offset]


def _track_args(_abi):
    a = _abi.hcTrackArgs()
    a.sub_ransac_iters = 1
    a.settings = _abi.hcTrackSettings(80, 3, 4)
    for f in ("start_sols", "tracks", "start_params", "target_params", "diff_params", "unified_index",
              "converge", "infinity"):
        setattr(a, f, 0x1000)       # never dereferenced: validation fails first
    return a


def _group_args(_abi, **kw):
    g = _abi.hcGroupedAbortArgs()
    g.num_groups = 2
    for f in ("groups", "sample_group", "group_found", "trifocal_sols_batch_index"):
        setattr(g, f, 0x1000)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _gate(_abi, ratio, counts=None):
    j = _abi.hcJointGate()
    j.min_joint_ratio = ratio
    j.joint_inliers = counts
    return j


def test_gated_rejects_bad_arguments_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    fn = L.hc_trifocal_2op1p_30x30_track_abort_gated
    ws = int(L.hc_trifocal_workspace_size())
    dummy = C.c_void_p(0x1000)
    a = _track_args(_abi)
    ok = _gate(_abi, 0.3)
    assert fn(C.byref(a), C.byref(_group_args(_abi)), None, dummy, ws, None) == 1                 # null gate
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert fn(C.byref(a), C.byref(_group_args(_abi)), C.byref(_gate(_abi, bad)), dummy, ws, None) == 1, bad
    # whatever the grouped call rejects
    assert fn(C.byref(a), None, C.byref(ok), dummy, ws, None) == 1
    assert fn(None, C.byref(_group_args(_abi)), C.byref(ok), dummy, ws, None) == 1
    for f in ("groups", "group_found", "sample_group", "trifocal_sols_batch_index"):
        assert fn(C.byref(a), C.byref(_group_args(_abi, **{f: None})), C.byref(ok), dummy, ws, None) == 1, f
    assert fn(C.byref(a), C.byref(_group_args(_abi, num_groups=0)), C.byref(ok), dummy, ws, None) == 1
    # then the launch's own checks, in the grouped call's order
    assert fn(C.byref(a), C.byref(_group_args(_abi)), C.byref(ok), None, ws, None) == 2
    assert fn(C.byref(a), C.byref(_group_args(_abi)), C.byref(ok), dummy, ws - 1, None) == 2
    a.sub_ransac_iters = 0               # zero samples: a no-op success; a ratio > 1 is valid, the counts optional
    assert fn(C.byref(a), C.byref(_group_args(_abi)), C.byref(_gate(_abi, 2.0)), dummy, ws, None) == 0
    a.sub_ransac_iters = -1
    assert fn(C.byref(a), C.byref(_group_args(_abi)), C.byref(ok), dummy, ws, None) == 1


@pytest.mark.parametrize("gate", ["0.3", 1, True, [0.3], 0.0, -0.5, float("nan"), float("inf"), 1e-60])
def test_python_wrapper_rejects_a_bad_gate(gate):
    """gate must be a float (Python or numpy), finite and positive as a
    float32; the check comes before anything touches a device."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, tracker
    with pytest.raises(_abi.HCError):
        tracker.gate_ratio(gate)
    with pytest.raises(_abi.HCError):
        tracker.DeviceTracker.launch_grouped(None, None, None, gate=gate)
    with pytest.raises(_abi.HCError):
        tracker.DeviceTracker.track_grouped(None, None, gate=gate)


def test_python_wrapper_gate_value_is_the_float32():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import tracker
    assert tracker.gate_ratio(0.2) == float(np.float32(0.2)) != 0.2
    assert tracker.gate_ratio(np.float32(0.39)) == float(np.float32(0.39))
    assert tracker.gate_ratio(2.0) == 2.0
