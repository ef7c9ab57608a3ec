"""CPU tests of the pose refinement (include/refine/hc_pose_refine.h): the
numpy reference of the method (tests/refine_reference.py) on the committed
config-5 fixture and on noiseless scenes, and the host side of the two entry
points: exports, prototypes, struct layouts through the C compiler, argument
validation (no device is touched: validation fails first) and the Python
wrapper's own checks.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import refine_reference as RR
from checks import NOISE_SEED, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "refine", "hc_pose_refine.h")
POSE_KEYS = RR.POSE_KEYS


# ---- the reference on the fixture -------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_case(oracle, ransac0):
    """The winner of pose_joint_noisy1px_N100.npz as the oracle converts it to
    a pose, on the edgels of Triplet_Edgels_000 with the oracle's 1 px noise."""
    g = golden("pose_joint_noisy1px_N100")
    loc = oracle.add_pixel_noise(ransac0.locations, ransac0.K, 1.0, NOISE_SEED)
    i = int(np.nonzero(g["cand_ids"] == g["path"])[0][0])
    inl, sel = oracle.pose_support(g["cand_tracks"][i:i + 1], np.ones(1, np.uint8), loc, ransac0.K)
    assert inl[0].tolist() == g["inliers"][1:].tolist()
    loc.setflags(write=False)
    return dict(sel=sel, loc=loc, K=ransac0.K, joint=int(g["inliers"][0]), ref=RR.refine(sel, loc, ransac0.K))


def test_reference_scoring_is_the_oracles(oracle, fixture_case):
    """The float32 restatement of the 2 px test gives the oracle's per-view
    counts and the fixture's joint count and mask for the input pose."""
    c = fixture_case
    g = golden("pose_joint_noisy1px_N100")
    m21, m31 = RR.score(c["loc"], c["K"], tuple(c["sel"][k] for k in POSE_KEYS))
    assert (int(m21.sum()), int(m31.sum())) == (c["sel"]["inliers21"], c["sel"]["inliers31"])
    assert int((m21 & m31).sum()) == c["joint"] == 1133
    bits = np.unpackbits(g["mask"].view(np.uint8), bitorder="little")[:len(m21)].astype(bool)
    assert np.array_equal(m21 & m31, bits)


def test_reference_on_the_fixture(oracle, ransac0, fixture_case):
    c, r = fixture_case, fixture_case["ref"]
    h = r["joint_history"]
    assert r["status"] == 0 and r["iterations_run"] == 10
    assert h[0] == 1133 and (h[:11] >= 0).all() and (h[11:] == -1).all()
    assert (np.diff(h[:r["best_iteration"] + 1]) >= 0).all()
    assert r["inliers"] == h[r["best_iteration"]] == h[:11].max()
    # the float64-scored prototype gave 3640; the float32-scored reference gives
    assert r["inliers"] == 3640 and r["best_iteration"] == 6
    assert r["inliers"] >= 3500
    before, _ = oracle.pose_residuals(ransac0.pose21, ransac0.pose31, c["sel"])
    after, ok = oracle.pose_residuals(ransac0.pose21, ransac0.pose31, r)
    assert abs(before[0] - 0.0773) < 1e-4 and abs(before[1] - 0.0443) < 1e-4
    assert ok and after[0] < 0.02 and after[1] < 0.02
    assert (r["rms_px_out"] < r["rms_px_in"]).all() and (r["rms_px_out"] < 2.0).all()
    # the edgels another summation order may flip: few enough to bound the GPU's count by
    assert 0 < RR.borderline(c["loc"], c["K"], r["pose64"]) <= 0.01 * len(c["loc"])


def test_reference_returns_the_input_when_nothing_is_better(fixture_case):
    """Too few inliers at iterate 0: the input floats, bit for bit, and the status."""
    c = fixture_case
    r = RR.refine(c["sel"], c["loc"][:15], c["K"])
    assert r["status"] == RR.TOO_FEW and r["iterations_run"] == r["best_iteration"] == 0
    for k in POSE_KEYS:
        assert r[k].tobytes() == np.asarray(c["sel"][k], np.float32).tobytes()


@pytest.mark.parametrize("E", [257, 2049])
def test_reference_noiseless_recovery(ransac0, E):
    """The GT pose perturbed by 3e-4 rad comes back to the pose that refining
    the GT pose itself gives, within 1e-6 in |dR|_F and |dt|_2 (float64 states:
    an arccos would be blind below 1e-4)."""
    loc = ransac0.locations[:E]
    gt = RR.gt_pose(ransac0)
    start = RR.perturbed(gt)
    assert 2e-4 < RR.pose_distance(gt, start) < 1e-3
    a = RR.refine(gt, loc, ransac0.K)
    b = RR.refine(start, loc, ransac0.K)
    assert a["status"] == b["status"] == 0 and a["inliers"] == b["inliers"] == E
    for v in range(2):
        assert np.linalg.norm(a["pose64"][v][0] - b["pose64"][v][0]) < 1e-6
        assert np.linalg.norm(a["pose64"][v][1] - b["pose64"][v][1]) < 1e-6
    assert RR.pose_distance(a, b) < 1e-6


def test_reference_jacobian_against_the_closed_form(ransac0):
    """The central differences against the derivative written out (the form the
    kernel sums): the two normal matrices agree to the differences' own error."""
    gt = RR.gt_pose(ransac0)
    l64 = ransac0.locations[:64].astype(np.float64)
    R, t = np.asarray(gt["R21"], np.float64).reshape(3, 3), np.asarray(gt["t21"], np.float64)
    g, h = l64[:, 0:2], l64[:, 2:4]
    A, grad, _ = RR.normal_equations(g, h, R, t, ransac0.K)
    K0, K4 = float(ransac0.K[0]), float(ransac0.K[4])
    b1, b2 = RR.tangent_basis(t)
    c = R[:, 2]
    J = np.zeros((64, 2, 5))
    for e in range(64):
        hh, gg = np.array([h[e, 0], h[e, 1], 1.0]), np.array([g[e, 0], g[e, 1], 1.0])
        a, m = c @ hh, R @ gg
        den = 1.0 - m[2] * a
        rho = (t[2] * a - c @ t) / den
        q = m * rho + t
        for d in range(5):
            w = np.eye(3)[d] if d < 3 else np.zeros(3)
            dt = np.zeros(3) if d < 3 else (b1, b2)[d - 3]
            dc, dm = np.cross(w, c), np.cross(w, m)
            da = dc @ hh
            dnum = dt[2] * a + t[2] * da - (dc @ t + c @ dt)
            dden = -(dm[2] * a + m[2] * da)
            drho = (dnum - rho * dden) / den
            dq = dm * rho + m * drho + dt
            J[e, 0, d] = K0 * (dq[0] - q[0] / q[2] * dq[2]) / q[2]
            J[e, 1, d] = K4 * (dq[1] - q[1] / q[2] * dq[2]) / q[2]
    J = J.reshape(-1, 5)
    assert np.abs(J.T @ J - A).max() <= 1e-7 * np.abs(A).max()


# ---- the ABI of the refinement header -----------------------------------------------------

def _prototypes():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M):
        out[name] = (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
    return out


def test_symbols_exported_declared_and_bound():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    protos = _prototypes()
    assert set(protos) == set(_abi.REFINE_DECLARED_SYMBOLS) == {"hc_trifocal_pose_refine",
                                                                "hc_trifocal_pose_refine_grouped"}
    for s in _abi.REFINE_SIGNATURES:
        ret, params = protos[s.name]
        assert ret == "hcStatus" and s.restype is C.c_int
        assert len(params) == len(s.argtypes), s.name
        for k, (p, t) in enumerate(zip(params, s.argtypes)):
            if "*" in p or p.startswith("hcStream "):
                assert t is C.c_void_p or issubclass(t, C._Pointer), (s.name, k)
            else:
                assert p.startswith("int ") and t is C.c_int, (s.name, k, p)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    exported = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert set(_abi.REFINE_DECLARED_SYMBOLS) <= exported
    L = _abi.lib()
    for s in _abi.REFINE_SIGNATURES:
        fn = getattr(L, s.name)
        assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    # additive: no struct of the other headers changed
    assert L.hc_trifocal_abi_version() == _abi.ABI_VERSION == 2
    assert "#define HC_TRIFOCAL_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "hc_trifocal.h")).read()


def test_struct_mirrors_match_the_header_by_the_c_compiler(tmp_path):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    structs = (_abi.hcRefineSettings, _abi.hcRefineReport)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "refine/hc_pose_refine.h"', 'int main(void) {']
    for s in structs:
        args = "".join(f", offsetof({s.__name__}, {f[0]})" for f in s._fields_)
        lines.append(f'    printf("{"%zu " * (1 + len(s._fields_))}\\n", sizeof({s.__name__}){args});')
    lines += ['    printf("%d %d %d %d\\n", HC_REFINE_MAX_ITERATIONS, HC_REFINE_NONE, HC_REFINE_TOO_FEW, '
              'HC_REFINE_SINGULAR);', '    return 0;', '}', '']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    for s, line in zip(structs, out):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_], s.__name__
    assert (C.sizeof(_abi.hcRefineSettings), C.sizeof(_abi.hcRefineReport)) == (16, 176)
    assert _abi.REFINE_REPORT_BYTES == 176
    assert [int(v) for v in out[2].split()] == [_abi.HC_REFINE_MAX_ITERATIONS, _abi.HC_REFINE_NONE,
                                                _abi.HC_REFINE_TOO_FEW, _abi.HC_REFINE_SINGULAR] == [32, 1, 2, 4]


def _settings(iterations=0, min_inliers=0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    s = _abi.hcRefineSettings()
    s.iterations, s.min_inliers = iterations, min_inliers
    return s


BAD_SETTINGS = [(-1, 0), (33, 0), (1 << 30, 0), (0, -1), (0, 1), (0, 5), (10, -16)]


def test_invalid_arguments_are_rejected_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    INVALID = 1
    p = C.c_void_p(0x1000)   # never dereferenced: validation fails first
    # hc_trifocal_pose_refine(in, E, locations, K, settings, out, report, stream)
    good = [p, 100, p, p, None, p, None, None]
    for i, bad in ((0, None), (1, 0), (1, -1), (2, None), (3, None), (5, None)):
        a = list(good)
        a[i] = bad
        assert L.hc_trifocal_pose_refine(*a) == INVALID, (i, bad)
    for it, mi in BAD_SETTINGS:
        a = list(good)
        a[4] = C.byref(_settings(it, mi))
        assert L.hc_trifocal_pose_refine(*a) == INVALID, (it, mi)
    # hc_trifocal_pose_refine_grouped(T, groups, in, settings, out, reports, stream)
    good = [3, p, p, None, p, None, None]
    for i, bad in ((0, 0), (0, -1), (1, None), (2, None), (4, None)):
        a = list(good)
        a[i] = bad
        assert L.hc_trifocal_pose_refine_grouped(*a) == INVALID, (i, bad)
    for it, mi in BAD_SETTINGS:
        a = list(good)
        a[3] = C.byref(_settings(it, mi))
        assert L.hc_trifocal_pose_refine_grouped(*a) == INVALID, (it, mi)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(iterations=33), dict(iterations=-1), dict(iterations=2.0),
                                dict(iterations=True), dict(min_inliers=5), dict(min_inliers=0),
                                dict(min_inliers="16")])
def test_python_wrapper_rejects_bad_settings(kw):
    """The check comes before anything touches a device."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    with pytest.raises(_abi.HCError):
        pose.launch_refine_joint(None, None, None, **kw)
    with pytest.raises(_abi.HCError):
        pose.launch_refine_joint_grouped(None, None, **kw)


def test_report_dict_decodes_the_struct():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    r = _abi.hcRefineReport()
    r.status, r.iterations_run, r.best_iteration = 6, 3, 2
    r.joint_history[:] = [5, 7, 9, 8] + [-1] * 29
    r.rms_px_in[:] = [1.5, 1.25]
    r.rms_px_out[:] = [0.5, 0.75]
    d = pose.refine_report_dict(np.frombuffer(bytes(r), np.uint8))
    assert (d["status"], d["none"], d["too_few"], d["singular"]) == (6, False, True, True)
    assert (d["iterations_run"], d["best_iteration"]) == (3, 2)
    assert d["joint_history"].tolist() == [5, 7, 9, 8] + [-1] * 29
    assert d["rms_px_in"].tolist() == [1.5, 1.25] and d["rms_px_out"].tolist() == [0.5, 0.75]
