"""CPU tests of the adaptive sample limit's host side
(include/adaptive/hc_trifocal_adaptive.h): the hcAdaptiveGate layout through the
C compiler, hc_ransac_need_table against a Python restatement of the rule, the
mode switch on hcJointGate::pad with the argument checks made before any device
work, and the Python wrappers (TripletBatch.sample_ordinal, AdaptiveStop)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adaptive", "hc_trifocal_adaptive.h")
GATED = "hc_trifocal_2op1p_30x30_track_abort_gated"
FIELDS = ("head", "need", "need_offset", "sample_ordinal", "group_limit")


# ---- the ABI of the header ------------------------------------------------------------------

def test_header_declares_one_host_function_and_no_launch():
    """The header against _abi.ADAPTIVE_SIGNATURES, the exports and the bound
    function; it adds no prototype to include/*.h and none with a stream."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {name: (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
              for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M)}
    assert set(protos) == set(_abi.ADAPTIVE_DECLARED_SYMBOLS) == {"hc_ransac_need_table"}
    ret, params = protos["hc_ransac_need_table"]
    assert ret == "hcStatus"
    assert params == ["int num_edgels", "double confidence", "int min_samples", "int max_samples", "int32_t *need"]
    assert "hcStream" not in src
    (s,) = _abi.ADAPTIVE_SIGNATURES
    assert s.restype is C.c_int and tuple(s.argtypes) == (C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p)
    fn = getattr(_abi.lib(), s.name)
    assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert "hc_ransac_need_table" in {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    others = _abi.DECLARED_SYMBOLS + _abi.P2C_DECLARED_SYMBOLS + _abi.REFINE_DECLARED_SYMBOLS + \
        _abi.TOPK_DECLARED_SYMBOLS + _abi.LU_DECLARED_SYMBOLS
    assert "hc_ransac_need_table" not in others
    # additive: no struct of hc_trifocal.h changed
    assert _abi.lib().hc_trifocal_abi_version() == _abi.ABI_VERSION == 2
    assert C.sizeof(_abi.hcJointGate) == 16


def test_adaptive_gate_layout_by_the_c_compiler(tmp_path):
    """sizeof(hcAdaptiveGate) and every offsetof equal the ctypes mirror's, head
    is at offset 0 (the caller casts the struct's address to the head's type),
    and the magic value is the header's."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    offs = "".join(f", offsetof(hcAdaptiveGate, {f})" for f in FIELDS)
    src = tmp_path / "adaptive.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "adaptive/hc_trifocal_adaptive.h"\n'
                   'int main(void) { hcAdaptiveGate g; const hcJointGate *h = (const hcJointGate *)&g;\n'
                   f'printf("{"%zu " * 6}%ld %d\\n", sizeof(hcAdaptiveGate){offs}, (long)HC_GATE_ADAPTIVE, '
                   '(const void *)h == (const void *)&g.head); return 0; }\n')
    exe = tmp_path / "adaptive"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True,
                                          timeout=30).stdout.split()]
    g = _abi.hcAdaptiveGate
    assert [f[0] for f in g._fields_] == list(FIELDS)
    assert out[:6] == [C.sizeof(g)] + [getattr(g, f).offset for f in FIELDS] == [48, 0, 16, 24, 32, 40]
    assert out[6] == _abi.HC_GATE_ADAPTIVE == 0x41445031 == int.from_bytes(b"ADP1", "big")
    assert out[7] == 1
    assert g.head.offset == 0 and g._fields_[0][1] is _abi.hcJointGate


# ---- hc_ransac_need_table ----------------------------------------------------------------------

def need_ref(E, p, lo, hi):
    """The header's rule, restated: everything in double."""
    out = []
    for c in range(E + 1):
        w = c / E
        q = 1.0 - w * w * w
        if q <= 0.0:
            n = 0
        elif q >= 1.0:
            n = hi
        else:
            v = math.log(1.0 - p) / math.log(q)
            n = math.ceil(v) if math.isfinite(v) else hi
        out.append(min(max(n, lo), hi))
    return np.array(out, np.int64)


@pytest.mark.parametrize("p", [0.5, 0.99, 0.999])
@pytest.mark.parametrize("E", [1, 2, 33, 5117])
def test_need_table_against_the_restatement(E, p):
    """Entries small enough for the two bounds to be computable: at n <= 10^6
    the power's rounding error, about n * 2^-53, stays below the 1e-9 allowed."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import tracker
    lo, hi = 1, 10 ** 6
    need = tracker.need_table(E, p, lo, hi)
    assert need.dtype == np.int32 and need.shape == (E + 1,)
    assert np.array_equal(need, need_ref(E, p, lo, hi))
    assert (np.diff(need) <= 0).all()
    assert need[0] == hi and need[E] == lo
    checked = 0
    for c in range(E + 1):
        n = int(need[c])
        if lo < n < hi:        # unclamped
            q = 1.0 - (c / E) ** 3
            assert q ** n <= (1.0 - p) * (1.0 + 1e-9), (c, n)
            assert q ** (n - 1) >= (1.0 - p) * (1.0 - 1e-9), (c, n)
            checked += 1
    assert checked > 0 or E <= 2
    # other clamps: the same rule
    assert np.array_equal(tracker.need_table(E, p, 3, 100), need_ref(E, p, 3, 100))
    assert np.array_equal(tracker.need_table(E, p, 7, 7), np.full(E + 1, 7))


def test_need_table_spot_values():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import tracker
    need = tracker.need_table(5117, 0.99, 1, 2 ** 31 - 1)
    assert (need[1024], need[1133], need[1996], need[3640]) == (573, 422, 76, 11)
    assert need[0] == 2 ** 31 - 1 and need[5117] == 1
    half = tracker.need_table(5117, 0.5, 1, 100)
    assert half[697] == 100 and half[1133] == 64


def test_need_table_rejects_bad_arguments():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, tracker
    fn = _abi.lib().hc_ransac_need_table
    buf = np.zeros(8, np.int32)
    p = _abi.ptr(buf)
    assert fn(7, 0.99, 1, 10, p) == 0
    for E in (0, -1):
        assert fn(E, 0.99, 1, 10, p) == 1
    for conf in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert fn(7, conf, 1, 10, p) == 1, conf
    for lo, hi in ((0, 10), (-3, 10), (5, 4)):
        assert fn(7, 0.99, lo, hi, p) == 1, (lo, hi)
    assert fn(7, 0.99, 1, 10, None) == 1
    with pytest.raises(_abi.HCError):
        tracker.need_table(0, 0.99)
    with pytest.raises(_abi.HCError):
        tracker.need_table(7, 1.0)


# ---- the mode switch --------------------------------------------------------------------------

def _blocks(_abi, pad, tables=0x1000, **null):
    a = _abi.hcTrackArgs()
    a.sub_ransac_iters = 1
    a.settings = _abi.hcTrackSettings(80, 3, 4)
    for f in ("start_sols", "tracks", "start_params", "target_params", "diff_params", "unified_index",
              "converge", "infinity"):
        setattr(a, f, 0x1000)       # never dereferenced: validation fails first
    g = _abi.hcGroupedAbortArgs()
    g.num_groups = 2
    for f in ("groups", "sample_group", "group_found", "trifocal_sols_batch_index"):
        setattr(g, f, 0x1000)
    ag = _abi.hcAdaptiveGate()
    ag.head.min_joint_ratio = 2.0
    ag.head.pad = pad
    for f in FIELDS[1:]:
        setattr(ag, f, None if null.get(f) else tables)
    return a, g, ag


def _call(_abi, a, g, ag, workspace):
    L = _abi.lib()
    return getattr(L, GATED)(C.byref(a), C.byref(g), C.cast(C.pointer(ag), C.POINTER(_abi.hcJointGate)), workspace,
                             int(L.hc_trifocal_workspace_size()), None)


def test_magic_pad_selects_the_adaptive_gate_and_validates_it():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    dummy = C.c_void_p(0x1000)
    for f in FIELDS[1:]:
        # a NULL table pointer is rejected before the workspace is looked at
        assert _call(_abi, *_blocks(_abi, _abi.HC_GATE_ADAPTIVE, **{f: True}), dummy) == 1, f
        assert _call(_abi, *_blocks(_abi, _abi.HC_GATE_ADAPTIVE, **{f: True}), None) == 1, f
    # a complete adaptive gate goes on to the launch's own checks, in their order
    assert _call(_abi, *_blocks(_abi, _abi.HC_GATE_ADAPTIVE), None) == 2
    a, g, ag = _blocks(_abi, _abi.HC_GATE_ADAPTIVE)
    a.sub_ransac_iters = 0
    assert _call(_abi, a, g, ag, dummy) == 0
    ag.head.min_joint_ratio = 0.0           # the ratio keeps its check
    assert _call(_abi, a, g, ag, dummy) == 1


@pytest.mark.parametrize("pad", [7, 0, -1, 0x41445030, 0x31504441])
def test_any_other_pad_is_the_ratio_gate(pad):
    """The same block with NULL table pointers: what the ratio gate returns."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    nulls = {f: True for f in FIELDS[1:]}
    assert _call(_abi, *_blocks(_abi, pad, **nulls), None) == 2          # a NULL workspace
    a, g, ag = _blocks(_abi, pad, **nulls)
    a.sub_ransac_iters = 0
    assert _call(_abi, a, g, ag, C.c_void_p(0x1000)) == 0
    g.group_found = None
    assert _call(_abi, a, g, ag, C.c_void_p(0x1000)) == 1


# ---- the Python wrappers ----------------------------------------------------------------------

def test_sample_ordinal_of_an_interleaved_and_a_blocked_batch(problem, ransac0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    ds = [ransac0, ransac0, ransac0]
    b = TripletBatch(problem, ds, samples_per_triplet=[3, 1, 2], interleave=True)
    assert b.sample_group.tolist() == [0, 1, 2, 0, 2, 0]
    assert b.sample_ordinal.tolist() == [0, 0, 0, 1, 1, 2] and b.sample_ordinal.dtype == np.int32
    b = TripletBatch(problem, ds, samples_per_triplet=[3, 1, 2])
    assert b.sample_group.tolist() == [0, 0, 0, 1, 2, 2]
    assert b.sample_ordinal.tolist() == [0, 1, 2, 0, 0, 1]
    for t in range(3):   # a triplet's rows carry 0, 1, 2, ... in launch order
        assert b.sample_ordinal[b.index[t]].tolist() == list(range(len(b.index[t])))


@pytest.mark.parametrize("kw", [dict(confidence=0.0), dict(confidence=1.0), dict(confidence=-0.1),
                                dict(confidence=float("nan")), dict(confidence="0.9"), dict(confidence=1),
                                dict(confidence=True), dict(min_samples=0), dict(min_samples=-2),
                                dict(min_samples=1.5), dict(min_samples=True), dict(max_samples=0),
                                dict(min_samples=5, max_samples=4), dict(tables=[]), dict(tables=np.zeros(5, np.int32)),
                                dict(tables=[np.zeros((2, 2), np.int32)]), dict(tables=[np.array([1.0, 2.0])]),
                                dict(tables=[np.array([1], np.int32)]), dict(tables=[np.array([-1, 3], np.int32)]),
                                dict(tables=3)])
def test_adaptive_stop_rejects(kw):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, tracker
    with pytest.raises(_abi.HCError):
        tracker.AdaptiveStop(**kw)


def test_adaptive_stop_tables_and_wrapper_checks():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, tracker
    a = tracker.AdaptiveStop()
    assert (a.confidence, a.min_samples, a.max_samples, a.tables) == (0.99, 1, None, None)
    # max_samples defaults to the triplet's own sample count
    t5, t33 = a.host_tables([5, 33], [100, 7])
    assert np.array_equal(t5, tracker.need_table(5, 0.99, 1, 100)) and np.array_equal(t33, tracker.need_table(33, 0.99, 1, 7))
    own = tracker.AdaptiveStop(tables=[np.arange(6)[::-1], np.full(34, 9)])
    got = own.host_tables([5, 33], [100, 7])
    assert got[0].dtype == np.int32 and got[0].tolist() == [5, 4, 3, 2, 1, 0] and got[1].tolist() == [9] * 34
    for ec in ([5], [5, 32], [4, 33]):
        with pytest.raises(_abi.HCError):
            own.host_tables(ec, [1] * len(ec))
    # the wrappers' checks come in today's order (gate first), before anything touches a device
    for bad in ("x", 0.99, True, {}):
        with pytest.raises(_abi.HCError):
            tracker.DeviceTracker.launch_grouped(None, None, None, adaptive=bad)
        with pytest.raises(_abi.HCError):
            tracker.DeviceTracker.track_grouped(None, None, adaptive=bad)
    with pytest.raises(_abi.HCError, match="gate"):
        tracker.DeviceTracker.launch_grouped(None, None, None, gate=0.0, adaptive="x")
    with pytest.raises(_abi.HCError):
        tracker.DeviceTracker.track_grouped(None, None, limit=[3])
