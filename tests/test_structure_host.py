"""CPU tests of the structure stage's host side
(include/structure/hc_pose_structure.h): the header declaring no function, the
struct layouts and macro values through the C compiler, the mode switch on
hcRefineSettings::pad with its argument checks made before any device work, the
Python wrappers' own checks, and the numpy reference of the rule
(tests/structure_reference.py) under the ground-truth pose on the clean
datasets 000 and 050, through the three-view reference's chain on the config-5
fixture, and on the degenerate tangents.

The reference's figures (printed by test_ground_truth_pose_on_clean_data):
  dataset 000, s = 1.185279:   5117 of 5117, err3_px <= 2.72e-4, sin3 <= 2.47e-6 (fp64 9.5e-15), 46 without a tangent
  dataset 050, s = 0.82176995: 5117 of 5117, err3_px <= 3.71e-4, sin3 <= 3.39e-6 (fp64 6.9e-15), 72 without a tangent
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import refine_reference as RR
import scale_reference as SR
import structure_reference as ST
from checks import NOISE_SEED, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "structure", "hc_pose_structure.h")
DATA = os.path.join(ROOT, "data", "RANSAC_Data", "trifocal_2op1p_30x30", "Synthetic")
INVALID = 1
REFINE_CALLS = ("hc_trifocal_pose_refine", "hc_trifocal_pose_refine_grouped", "hc_trifocal_pose_refine_topk",
                "hc_trifocal_pose_refine_topk_grouped")
NOT_A_TAG = (0x54563330, 0x5A5A5A5A, 1, 7)     # what the other tests put into pad[0] as "no mode"


# ---- the ABI of the header ------------------------------------------------------------------

def test_header_declares_structs_and_macros_only():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    text = open(HEADER).read()
    assert '#include "../threeview/hc_pose_threeview.h"' in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\b(hc_\w+)\s*\(", src) == []
    assert "hcStream" not in src and "hcStatus" not in src
    assert set(re.findall(r"\}\s*(\w+)\s*;", src)) == {"hcEdgel3D", "hcStructureReport", "hcRefineStructureSettings"}
    assert set(re.findall(r"#define\s+(HC_\w+)", src)) - {"HC_POSE_STRUCTURE_H"} == set(_abi.STRUCTURE_CONSTANTS)
    # additive: no struct of the other headers changed, and no symbol was added for it
    assert _abi.lib().hc_trifocal_abi_version() == _abi.ABI_VERSION == 2
    assert (C.sizeof(_abi.hcRefineSettings), C.sizeof(_abi.hcRefineReport), C.sizeof(_abi.hcTrifocalSelection),
            C.sizeof(_abi.hcScaleReport), C.sizeof(_abi.hcRefineScaleSettings), C.sizeof(_abi.hcThreeViewReport),
            C.sizeof(_abi.hcRefineThreeViewSettings)) == (16, 176, 136, 40, 32, 328, 48)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert not [ln for ln in exported.splitlines()
                if any(w in ln.lower() for w in ("structure", "edgel3d", "reconstruct"))]
    assert _abi.HC_REFINE_STRUCTURE == int.from_bytes(b"ST3D", "big")
    assert _abi.HC_REFINE_STRUCTURE not in NOT_A_TAG + (_abi.HC_REFINE_SCALE31, _abi.HC_REFINE_THREEVIEW, 0)


def test_struct_mirrors_and_constants_match_the_header_by_the_c_compiler(tmp_path):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    structs = (_abi.hcEdgel3D, _abi.hcStructureReport, _abi.hcRefineStructureSettings)
    names = sorted(_abi.STRUCTURE_CONSTANTS)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "structure/hc_pose_structure.h"', 'int main(void) {',
             '    hcRefineStructureSettings s; const hcRefineSettings *h = (const hcRefineSettings *)&s;']
    for s in structs:
        args = "".join(f", offsetof({s.__name__}, {f[0]})" for f in s._fields_)
        lines.append(f'    printf("{"%zu " * (1 + len(s._fields_))}\\n", sizeof({s.__name__}){args});')
    lines += [f'    printf("{"%ld " * len(names)}%d\\n", {", ".join(f"(long){n}" for n in names)}, '
              '(const void *)h == (const void *)&s.tv.head);', '    return 0;', '}', '']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    for s, line in zip(structs, out):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_], s.__name__
    assert tuple(C.sizeof(s) for s in structs) == (48, 32, 88)
    assert (_abi.EDGEL3D_BYTES, _abi.STRUCTURE_REPORT_BYTES) == (48, 32)
    assert _abi.hcRefineStructureSettings.tv.offset == 0
    assert _abi.hcRefineStructureSettings._fields_[0][1] is _abi.hcRefineThreeViewSettings
    assert [int(v) for v in out[3].split()] == [_abi.STRUCTURE_CONSTANTS[n] for n in names] + [1]
    assert (_abi.HC_STRUCTURE_ONLY, _abi.HC_EDGEL3D_TANGENT, _abi.HC_EDGEL3D_ORIENTED, _abi.HC_STRUCTURE_NONE) == \
        (1, 1, 2, 1)
    # the numpy record is the struct, field by field, and the reference's
    d = _abi.EDGEL3D_DTYPE
    assert d.itemsize == 48 and d == ST.DTYPE
    assert [(n, d.fields[n][1]) for n in d.names] == [(f[0], getattr(_abi.hcEdgel3D, f[0]).offset)
                                                      for f in _abi.hcEdgel3D._fields_]


def _settings(bits=0, iterations=0, scale=0x2000, reports=0x4000, mask=None, iterations3=0, pad=0, tangents=0x5000,
              offsets=None, edgels3d=0x6000, sreports=0x7000, min_sin_plane=0.0, max_sin3=0.0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    s = _abi.hcRefineStructureSettings()
    s.tv.head.iterations = iterations
    s.tv.head.pad[0] = _abi.HC_REFINE_STRUCTURE
    s.tv.head.pad[1] = bits
    s.tv.scale_reports, s.tv.reports, s.tv.transfer_mask = scale, reports, mask
    s.tv.iterations3, s.tv.pad = iterations3, pad
    s.tangents, s.edgel_offsets, s.edgels3d, s.reports = tangents, offsets, edgels3d, sreports
    s.min_sin_plane, s.max_sin3 = min_sin_plane, max_sin3
    return s


def _calls():
    """name -> (the arguments of a valid call with never-dereferenced pointers, the index of settings)."""
    p = C.c_void_p(0x1000)
    return {"hc_trifocal_pose_refine": ([p, 100, p, p, None, p, None, None], 4),
            "hc_trifocal_pose_refine_grouped": ([3, p, p, None, p, None, None], 3),
            "hc_trifocal_pose_refine_topk": ([4, p, 100, p, p, None, p, None, p, p, None], 5),
            "hc_trifocal_pose_refine_topk_grouped": ([3, p, 4, p, None, p, None, p, p, None], 4)}


def test_invalid_mode_arguments_are_rejected_before_any_device_work():
    """Every case is refused by the validation, which comes before the first
    launch: the pointers are never dereferenced."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    RS = C.POINTER(_abi.hcRefineSettings)
    ONLY = _abi.HC_STRUCTURE_ONLY
    assert set(_calls()) == set(REFINE_CALLS)
    for name, (good, i) in _calls().items():
        topk = "topk" in name
        grouped = "grouped" in name
        off = 0x8000 if grouped else None        # what a valid call of this kind passes
        wrong_off = None if grouped else 0x8000
        nan, inf = float("nan"), float("inf")

        def only(**kw):
            kw = dict(dict(bits=ONLY, scale=None, reports=None, offsets=off), **kw)
            return _settings(**kw)
        bad = [_settings(offsets=off, tangents=None), _settings(offsets=off, edgels3d=None),
               _settings(offsets=off, sreports=None),                                    # NULL buffers of the mode
               _settings(offsets=wrong_off),                                             # offsets: grouped calls only
               _settings(offsets=off, min_sin_plane=nan), _settings(offsets=off, max_sin3=nan),
               _settings(offsets=off, min_sin_plane=inf), _settings(offsets=off, max_sin3=-inf),
               _settings(offsets=off, min_sin_plane=-0.01), _settings(offsets=off, max_sin3=1.001),
               _settings(offsets=off, bits=4), _settings(offsets=off, bits=8), _settings(offsets=off, bits=-1),
               _settings(offsets=off, bits=1 << 30),                                     # undefined bits
               # the three-view header's own checks
               _settings(offsets=off, scale=None), _settings(offsets=off, reports=None),
               _settings(offsets=off, iterations3=33), _settings(offsets=off, iterations3=-1),
               _settings(offsets=off, pad=1), _settings(offsets=off, iterations=33), _settings(offsets=off, iterations=-1),
               # HC_STRUCTURE_ONLY: nothing of the other stages may be asked for
               only(iterations=1), only(scale=0x2000), only(reports=0x4000), only(mask=0x3000), only(iterations3=1),
               only(pad=1), only(bits=ONLY | 2), only(bits=ONLY | 4), only(tangents=None), only(edgels3d=None),
               only(sreports=None), only(offsets=wrong_off), only(min_sin_plane=nan), only(max_sin3=2.0)]
        if topk:
            bad.append(only())                                                           # the refine calls only
        else:
            bad.append(_settings(offsets=off, bits=2))                                   # the top-k calls only
        if name != "hc_trifocal_pose_refine":
            bad.append(_settings(offsets=off, mask=0x3000))                              # the single call only
        for n, s in enumerate(bad):
            a = list(good)
            a[i] = C.cast(C.pointer(s), RS)
            assert getattr(L, name)(*a) == INVALID, (name, n, s.tv.head.iterations, s.tv.head.pad[1])
        # the other arguments are still checked in the mode
        for s in (_settings(offsets=off),) + (() if topk else (only(),)):
            a = list(good)
            a[i] = C.cast(C.pointer(s), RS)
            a[0] = None if isinstance(good[0], C.c_void_p) else 0
            assert getattr(L, name)(*a) == INVALID, name


def test_python_wrappers_reject_bad_keywords_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    bad = [dict(structure=1), dict(structure="yes"), dict(tangents=np.zeros((4, 6), np.float32)),   # tangents need the mode
           dict(structure=True, min_sin_plane=0.0), dict(structure=True, max_sin3=1.5),
           dict(structure=True, min_sin_plane=float("nan")), dict(structure=True, max_sin3=True),
           dict(structure=True, min_sin_plane="0.05"), dict(structure=True, three_view=1),
           dict(structure=True, three_view_iterations=0), dict(structure=True, fit_scale=1)]
    for kw in bad:
        with pytest.raises(_abi.HCError):
            pose.launch_refine_joint(None, None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.refine_joint(None, None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.launch_refine_joint_grouped(None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.refine_joint_grouped(None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.launch_refine_topk([None, None], None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.refine_topk_grouped([None, None], None, 2, **kw)
        with pytest.raises(_abi.HCError):
            pose.select_refined(None, None, None, None, **kw)
    for kw in (dict(min_sin_plane=0.0), dict(max_sin3=-1.0)):
        with pytest.raises(_abi.HCError):
            pose.launch_reconstruct(None, None, None, None, **kw)
    with pytest.raises(_abi.HCError):
        pose.launch_refine_topk([None, None], None, None, structure=True, transfer_mask=True)   # as with three_view


def test_report_dict_records_and_the_text_writer(tmp_path):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    r = _abi.hcStructureReport()
    r.status, r.count, r.tangents, r.oriented, r.scale31 = 0, 3, 2, 1, 1.1875
    d = pose.structure_report_dict(np.frombuffer(bytes(r), np.uint8))
    assert d == dict(status=0, none=False, count=3, tangents=2, oriented=1, scale31=np.float32(1.1875))
    r.status = _abi.HC_STRUCTURE_NONE
    assert pose.structure_report_dict(np.frombuffer(bytes(r), np.uint8))["none"]
    rec = np.zeros(2, pose.EDGEL3D_DTYPE)
    rec["edgel"], rec["flags"] = [4, 9], [3, 0]
    rec["X"][0], rec["T"][0] = [0.1, -0.25, 2.0], [0.0, 0.6, 0.8]
    rec["err3_px"], rec["sin_plane"], rec["sin3"] = [0.5, 1.25], [0.75, 0.01], [np.float32(1e-3), 1.0]
    path = tmp_path / "edgels3d.txt"
    pose.write_edgels3d(str(path), rec)
    lines = path.read_text().splitlines()
    assert len(lines) == 2 and lines[1] == "9 0 0 0 0 0 0 1.25 " + "%.9g" % np.float32(0.01) + " 1 0"
    got = lines[0].split()
    assert len(got) == 11 and got[0] == "4" and got[-1] == "3"
    back = np.array([float(v) for v in got[1:10]], np.float32)          # %.9g round-trips a float32
    assert back.tobytes() == np.concatenate([rec["X"][0], rec["T"][0], [rec["err3_px"][0], rec["sin_plane"][0],
                                                                        rec["sin3"][0]]]).astype(np.float32).tobytes()


def test_triplet_batch_carries_the_tangents(problem, ransac0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    b = TripletBatch(problem, [ransac0, ransac0], seeds=0, samples_per_triplet=1, edgel_counts=[17, None])
    assert [t.shape for t in b.tangents] == [(17, 6), ransac0.tangents.shape]
    assert np.array_equal(b.tangents[0], ransac0.tangents[:17]) and b.tangents[0].dtype == np.float32
    assert np.array_equal(b.locations[0], ransac0.locations[:17])


# ---- the reference -------------------------------------------------------------------------------

def _read64(index):
    """A dataset's text files in double: loc (E, 6), tan (E, 6), the pose as a
    dict (the files' translations are unit), K, and the scale every edgel
    proposes under it (the GT files do not hold it: step 2's s_e in double, the
    median of proposals that agree to 1e-9)."""
    rows = np.loadtxt(os.path.join(DATA, "Triplet_Edgels", f"Triplet_Edgels_{index:03d}.txt"), dtype=np.float64)
    loc = rows[:, [0, 1, 4, 5, 8, 9]]
    tan = rows[:, [2, 3, 6, 7, 10, 11]]
    K = np.loadtxt(os.path.join(DATA, "Intrinsic_Matrix.txt"), dtype=np.float64).reshape(9)
    p = {}
    for v in ("21", "31"):
        P = np.loadtxt(os.path.join(DATA, f"GT_Poses{v}", f"GT_Poses{v}_{index:03d}.txt"), dtype=np.float64).reshape(12)
        p["R" + v], p["t" + v] = P[:9], P[9:] / np.linalg.norm(P[9:])
    pose = {k: p[k] for k in RR.POSE_KEYS}
    _, _, s_e, _ = SR._edgels(loc, K, SR._pose(pose, np.float64), np.float64)
    s = float(np.median(s_e))
    assert np.abs(s_e - s).max() < 1e-9 * s
    return loc, tan, pose, K, s


@pytest.mark.parametrize("index", [0, 50])
def test_ground_truth_pose_on_clean_data(index):
    """The GT pose with the voted scale explains every edgel, and the
    reprojected 3D tangent lines up with view 3's, which no stage fits to.  The
    bounds are 30 times the figures of the prototype that fixed the rule."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data
    d = load_ransac_data(index)
    gt = RR.gt_pose(d)
    s = SR.fit(gt, d.locations, d.K)["scale31"]
    rec, rep = ST.reconstruct(gt, s, d.locations, d.tangents, d.K)
    E = len(d.locations)
    t = (rec["flags"] & ST.TANGENT) != 0
    loc64, tan64, gt64, K64, s64 = _read64(index)
    assert np.array_equal(loc64.astype(np.float32), d.locations) and np.array_equal(tan64.astype(np.float32), d.tangents)
    rec64, rep64 = ST.reconstruct64(gt64, s64, loc64, tan64, K64)
    print(f"dataset {index:03d}: s = {s!r} (fp64 {s64!r}), count {rep['count']} of {E}, tangents {rep['tangents']}, "
          f"oriented {rep['oriented']}, largest err3_px {rec['err3_px'].max():.3e}, largest sin3 with a tangent "
          f"{rec['sin3'][t].max():.3e}, median {np.median(rec['sin3'][t]):.3e}, fp64 on the same entries "
          f"{rec64['sin3'][t].max():.3e}, without a tangent {int((~t).sum())}, smallest sin_plane with one "
          f"{rec['sin_plane'][t].min():.4f}")
    assert rep["status"] == 0 and rep["count"] == E == len(rec) and np.array_equal(rec["edgel"], np.arange(E))
    assert rec["err3_px"].max() < 0.01
    assert rec["sin3"][t].max() < 1e-4
    assert int((~t).sum()) <= 0.02 * E
    assert np.array_equal(rec64["edgel"], rec["edgel"]) and rec64["sin3"][t].max() < 1e-9
    assert rep["tangents"] == int(t.sum()) == rep["oriented"] and rep["scale31"].tobytes() == np.float32(s).tobytes()
    # the entries without a tangent are the rule's step 4
    assert (rec["sin_plane"][~t] < np.float32(0.05)).all() and (rec["sin_plane"][t] >= np.float32(0.05)).all()
    assert not rec["T"][~t].any() and (rec["sin3"][~t] == 1.0).all() and (rec["flags"][~t] == 0).all()
    # a unit tangent whose image in view 1 points as the observed one, and a point in front of the camera
    assert np.abs(np.linalg.norm(rec["T"][t].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    g, a, T = d.locations[t, 0:2], d.tangents[t, 0:2], rec["T"][t]
    assert (((T[:, 0] - T[:, 2] * g[:, 0]) * a[:, 0] + (T[:, 1] - T[:, 2] * g[:, 1]) * a[:, 1]) >= 0).all()
    assert (rec["X"][:, 2] > 0).all() and not rec["pad"].any()
    assert np.abs(rec["X"].astype(np.float64) - rec64["X"]).max() < 1e-3 * np.abs(rec64["X"]).max()


def test_config5_fixture_through_the_reference_chain(oracle, ransac0):
    """The three-view reference's chain on the fixture, then the structure of
    the pose it returns: W is its transfer mask, in order."""
    import threeview_reference as TV
    from trifocal_pose_estimation_using_improved_gpuhc_amd import synthcurves
    g = golden("pose_joint_noisy1px_N100")
    noisy = synthcurves.noisy(ransac0, 1.0, NOISE_SEED)
    loc = oracle.add_pixel_noise(ransac0.locations, ransac0.K, 1.0, NOISE_SEED)
    assert np.array_equal(loc, noisy.locations)
    i = int(np.nonzero(g["cand_ids"] == g["path"])[0][0])
    _, sel = oracle.pose_support(g["cand_tracks"][i:i + 1], np.ones(1, np.uint8), loc, ransac0.K)
    r = RR.refine(sel, loc, ransac0.K)
    p24 = np.concatenate([r[k].reshape(-1) for k in RR.POSE_KEYS])
    s2 = dict(R21=p24[0:9], t21=p24[9:12], R31=p24[12:21], t31=p24[21:24], inliers=int(r["inliers"]),
              inliers21=int(r["inliers21"]), inliers31=int(r["inliers31"]))
    s2["scale31"] = SR.fit(s2, loc, ransac0.K)["scale31"]         # stage 2: the vote
    tv = TV.refine3(s2, loc, ransac0.K)
    rec, rep = ST.reconstruct(tv, tv["scale31"], loc, noisy.tangents, ransac0.K)
    t = (rec["flags"] & ST.TANGENT) != 0
    o = (rec["flags"] & ST.ORIENTED) != 0
    print(f"fixture: count {rep['count']} of {len(loc)}, tangents {rep['tangents']}, oriented {rep['oriented']}, "
          f"median sin3 {np.median(rec['sin3'][t]):.3e}, 90th percentile {np.percentile(rec['sin3'][t], 90):.3e}")
    assert rep["count"] == tv["transfer_inliers"] == len(rec) and 0 < rep["count"] < len(loc)
    assert np.array_equal(rec["edgel"], np.nonzero(tv["mask"])[0])
    assert (rec["err3_px"] < 2.0).all() and rep["oriented"] == int(o.sum()) <= rep["tangents"] == int(t.sum())
    assert np.median(rec["sin3"][t]) < 0.05          # sigma = 1 px: the pose still orients most tangents
    assert (rec["sin3"][o] < np.float32(0.05)).all() and (rec["sin3"][t & ~o] >= np.float32(0.05)).all()
    # nothing to reconstruct
    for kw in (dict(has_path=False), dict(fitted=False)):
        none, nrep = ST.reconstruct(tv, 1.5, loc, noisy.tangents, ransac0.K, **kw)
        assert len(none) == 0 and nrep == dict(status=ST.NONE, count=0, tangents=0, oriented=0, scale31=np.float32(1.5))


def test_degenerate_tangents(ransac0):
    """A zero tangent in view 1, a view-2 tangent along the epipolar line (of
    an edgel whose 3D tangent lies in the epipolar plane, so that view 1's is
    along its epipolar line too) and a threshold of 1.0: no tangent, T = 0,
    sin3 = 1, and the point as before."""
    gt = RR.gt_pose(ransac0)
    loc = ransac0.locations[:64]
    s = SR.fit(gt, ransac0.locations, ransac0.K)["scale31"]
    base, brep = ST.reconstruct(gt, s, loc, ransac0.tangents[:64], ransac0.K)
    ok = np.nonzero((base["flags"] & ST.TANGENT) != 0)[0]
    assert brep["count"] == 64 and len(ok) >= 60
    e0, e1 = int(ok[0]), int(ok[1])
    tan = np.array(ransac0.tangents[:64])
    tan[e0, 0:2] = 0.0
    # edgel e1: a view-2 tangent along the epipolar line.  It is the image of a 3D tangent in the epipolar plane,
    # whose view-1 image lies along view 1's epipolar line; with any other view-1 tangent the two planes still
    # meet, in the viewing ray of gamma1, at a large angle.  Both are checked.
    R = gt["R21"].astype(np.float64).reshape(3, 3)
    t21 = gt["t21"].astype(np.float64)
    c2 = -R.T @ t21                                               # the centre of camera 2 in view 1's frame
    a = loc[e1, 0:2].astype(np.float64) - c2[:2] / c2[2]
    b = loc[e1, 2:4].astype(np.float64) - t21[:2] / t21[2]
    tan[e1, 2:4] = (b / np.linalg.norm(b)).astype(np.float32)
    ray, _ = ST.reconstruct(gt, s, loc, tan, ransac0.K)           # view 1's tangent as observed
    assert ray["sin_plane"][e1] > 0.05 and ray["flags"][e1] & ST.TANGENT
    X = ray["X"][e1].astype(np.float64)
    assert np.abs(np.cross(ray["T"][e1].astype(np.float64), X / np.linalg.norm(X))).max() < 1e-3
    tan[e1, 0:2] = (a / np.linalg.norm(a)).astype(np.float32)
    rec, rep = ST.reconstruct(gt, s, loc, tan, ransac0.K)
    print(f"zero tangent: sin_plane {rec['sin_plane'][e0]!r}; epipolar tangent: sin_plane {rec['sin_plane'][e1]!r}")
    assert rep["count"] == 64 and rep["tangents"] == brep["tangents"] - 2
    assert np.isnan(rec["sin_plane"][e0]) and rec["sin_plane"][e1] < 1e-3
    for e in (e0, e1):
        assert rec["flags"][e] == 0 and not rec["T"][e].any() and rec["sin3"][e] == 1.0
        assert rec["X"][e].tobytes() == base["X"][e].tobytes() and rec["err3_px"][e] == base["err3_px"][e]
    keep = np.setdiff1d(np.arange(64), [e0, e1])
    assert rec[keep].tobytes() == base[keep].tobytes()
    # min_sin_plane = 1.0: only exactly perpendicular planes would pass
    rec1, rep1 = ST.reconstruct(gt, s, loc, ransac0.tangents[:64], ransac0.K, min_sin_plane=1.0)
    assert rep1["count"] == 64 and rep1["tangents"] == rep1["oriented"] == 0
    assert not rec1["T"].any() and (rec1["sin3"] == 1.0).all() and not rec1["flags"].any()
    assert rec1["X"].tobytes() == base["X"].tobytes() and rec1["sin_plane"].tobytes() == base["sin_plane"].tobytes()
    # max_sin3 = 1.0 orients every defined tangent whose sine is below 1
    rec2, rep2 = ST.reconstruct(gt, s, loc, ransac0.tangents[:64], ransac0.K, max_sin3=1.0)
    assert rep2["oriented"] == rep2["tangents"] == brep["tangents"]
