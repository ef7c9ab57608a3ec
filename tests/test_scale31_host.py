"""CPU tests of the scale fit's host side (include/scale/hc_pose_scale.h): the
struct layouts and macro values through the C compiler, the header declaring no
function, the mode switch on hcRefineSettings::pad with its argument checks made
before any device work, the Python wrappers' own checks, and the numpy float32
reference of the rule (tests/scale_reference.py) against its float64 form on
the clean data and on the committed config-5 fixture."""
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
HEADER = os.path.join(ROOT, "include", "scale", "hc_pose_scale.h")
INVALID = 1
REFINE_CALLS = ("hc_trifocal_pose_refine", "hc_trifocal_pose_refine_grouped", "hc_trifocal_pose_refine_topk",
                "hc_trifocal_pose_refine_topk_grouped")


# ---- the ABI of the header ------------------------------------------------------------------

def test_header_declares_structs_and_macros_only():
    """No prototype, no stream: the fit is a mode of the refine calls, so the
    sets of entry points that the other host tests pin do not change."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"\b(hc_\w+)\s*\(", src) == []
    assert "hcStream" not in src and "hcStatus" not in src
    assert set(re.findall(r"\}\s*(\w+)\s*;", src)) == {"hcScaleReport", "hcRefineScaleSettings"}
    # additive: no struct of the other headers changed, and no symbol was added for it
    assert _abi.lib().hc_trifocal_abi_version() == _abi.ABI_VERSION == 2
    assert (C.sizeof(_abi.hcRefineSettings), C.sizeof(_abi.hcRefineReport), C.sizeof(_abi.hcTrifocalSelection)) == \
        (16, 176, 136)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert not [ln for ln in exported.splitlines() if "scale" in ln.lower()]


def test_struct_mirrors_match_the_header_by_the_c_compiler(tmp_path):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    structs = (_abi.hcScaleReport, _abi.hcRefineScaleSettings)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "scale/hc_pose_scale.h"', 'int main(void) {',
             '    hcRefineScaleSettings s; const hcRefineSettings *h = (const hcRefineSettings *)&s;']
    for s in structs:
        args = "".join(f", offsetof({s.__name__}, {f[0]})" for f in s._fields_)
        lines.append(f'    printf("{"%zu " * (1 + len(s._fields_))}\\n", sizeof({s.__name__}){args});')
    lines += ['    printf("%ld %d %d %d %d %d\\n", (long)HC_REFINE_SCALE31, HC_SCALE_ONLY, HC_SCALE_SELECT_BY_TRANSFER, '
              'HC_SCALE_NONE, HC_SCALE_NO_VOTER, (const void *)h == (const void *)&s.head);', '    return 0;', '}', '']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    for s, line in zip(structs, out):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_], s.__name__
    assert (C.sizeof(_abi.hcScaleReport), C.sizeof(_abi.hcRefineScaleSettings)) == (40, 32)
    assert _abi.SCALE_REPORT_BYTES == 40 and _abi.hcScaleReport.key.offset == 32
    assert _abi.hcRefineScaleSettings.head.offset == 0 and _abi.hcRefineScaleSettings._fields_[0][1] is _abi.hcRefineSettings
    assert [int(v) for v in out[2].split()] == [_abi.HC_REFINE_SCALE31, _abi.HC_SCALE_ONLY,
                                                _abi.HC_SCALE_SELECT_BY_TRANSFER, _abi.HC_SCALE_NONE,
                                                _abi.HC_SCALE_NO_VOTER, 1]
    assert _abi.HC_REFINE_SCALE31 == int.from_bytes(b"SC31", "big")
    assert (_abi.HC_SCALE_ONLY, _abi.HC_SCALE_SELECT_BY_TRANSFER, _abi.HC_SCALE_NONE, _abi.HC_SCALE_NO_VOTER) == \
        (1, 2, 1, 2)


def _settings(bits=0, iterations=0, reports=0x2000, mask=None, tag=None):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    s = _abi.hcRefineScaleSettings()
    s.head.iterations = iterations
    s.head.pad[0] = _abi.HC_REFINE_SCALE31 if tag is None else tag
    s.head.pad[1] = bits
    s.reports = reports
    s.transfer_mask = mask
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
    assert set(_calls()) == set(REFINE_CALLS)
    for name, (good, i) in _calls().items():
        topk = "topk" in name
        single = name == "hc_trifocal_pose_refine"
        bad = [_settings(reports=None),                                    # NULL reports
               _settings(bits=_abi.HC_SCALE_ONLY, iterations=10),          # scale-only with iterations
               _settings(bits=_abi.HC_SCALE_ONLY, iterations=1),
               _settings(bits=4), _settings(bits=-1), _settings(bits=1 << 30),   # undefined bits
               _settings(iterations=33), _settings(iterations=-1)]         # the head's own range still holds
        if not topk:
            bad.append(_settings(bits=_abi.HC_SCALE_SELECT_BY_TRANSFER))   # the top-k calls only
        if not single:
            bad.append(_settings(mask=0x3000))                             # the single call only
        for s in bad:
            a = list(good)
            a[i] = C.cast(C.pointer(s), RS)
            assert getattr(L, name)(*a) == INVALID, (name, s.head.iterations, s.head.pad[1], s.reports,
                                                     s.transfer_mask)
        # the other arguments are still checked in the mode
        a = list(good)
        a[i] = C.cast(C.pointer(_settings()), RS)
        a[0] = None if isinstance(good[0], C.c_void_p) else 0
        assert getattr(L, name)(*a) == INVALID, name


def test_python_wrappers_reject_bad_keywords_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    bad = [dict(transfer_mask=True), dict(fit_scale=1), dict(fit_scale="yes"), dict(fit_scale=True, transfer_mask=1)]
    for kw in bad:
        with pytest.raises(_abi.HCError):
            pose.launch_refine_joint(None, None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.launch_refine_joint_grouped(None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.select_refined(None, None, None, None, **kw)
    with pytest.raises(_abi.HCError):
        pose.launch_refine_joint_grouped(None, None, fit_scale=True, transfer_mask=True)   # one scene only
    for kw in (dict(select_by_transfer=True), dict(fit_scale=True, select_by_transfer=0)):
        with pytest.raises(_abi.HCError):
            pose.launch_refine_topk([None, None], None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.select_refined(None, None, None, None, **kw)
    with pytest.raises(TypeError):
        pose.launch_refine_joint(None, None, None, select_by_transfer=True)               # top-k only


def test_scale_report_dict_decodes_the_struct():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    r = _abi.hcScaleReport()
    r.status, r.num_voters, r.voter, r.transfer_inliers, r.tested, r.joint = 2, 7, 5039, 614, 1100, 1133
    r.scale_in, r.scale31, r.key = 22.75, 1.25, (614 << 32) | 5039
    d = pose.scale_report_dict(np.frombuffer(bytes(r), np.uint8))
    assert (d["status"], d["none"], d["no_voter"]) == (2, False, True)
    assert (d["num_voters"], d["voter"], d["transfer_inliers"], d["tested"], d["joint"]) == (7, 5039, 614, 1100, 1133)
    assert (float(d["scale_in"]), float(d["scale31"]), d["key"]) == (22.75, 1.25, (614 << 32) | 5039)


# ---- the reference against its float64 form ----------------------------------------------------

def test_reference_on_clean_data_gives_the_true_scale(ransac0):
    """Dataset 000, noiseless, under the GT poses: every edgel proposes the same
    scale, 1.1852790 in float64 (the GT files store unit translations: the
    number is not in them), and the float32 rule is within 1e-5 relative of it."""
    import scale_reference as SR
    gt = RR.gt_pose(ransac0)
    E = len(ransac0.locations)
    r32 = SR.fit(gt, ransac0.locations, ransac0.K)
    r64 = SR.fit64(gt, ransac0.locations, ransac0.K)
    print(f"clean: float32 {r32['scale31']!r} ({r32['transfer_inliers']} of {r32['tested']}), float64 {r64['scale31']!r}")
    assert abs(float(r64["scale31"]) - 1.1852790) < 1e-6
    assert abs(float(r32["scale31"]) - float(r64["scale31"])) <= 1e-5 * float(r64["scale31"])
    for r in (r32, r64):
        assert r["status"] == 0 and r["joint"] == r["tested"] == r["num_voters"] == r["transfer_inliers"] == E
        assert r["mask"].all() and (r["counts"] == E).all()
        assert r["voter"] == E - 1                    # all tied: the last voter
    assert r32["key"] == (E << 32) | (E - 1)


@pytest.fixture(scope="module")
def fixture_case(oracle, ransac0):
    """The joint winner of pose_joint_noisy1px_N100.npz as the oracle converts it
    to a pose, on the 5117 edgels with the oracle's 1 px noise."""
    g = golden("pose_joint_noisy1px_N100")
    loc = oracle.add_pixel_noise(ransac0.locations, ransac0.K, 1.0, NOISE_SEED)
    i = int(np.nonzero(g["cand_ids"] == g["path"])[0][0])
    _, sel = oracle.pose_support(g["cand_tracks"][i:i + 1], np.ones(1, np.uint8), loc, ransac0.K)
    x = g["cand_tracks"][i][:, 0].astype(np.float64)
    ratio = float(np.linalg.norm(x[21:24]) / np.linalg.norm(x[18:21]))
    return dict(sel=sel, loc=loc, K=ransac0.K, ratio=ratio)


def test_reference_on_the_noisy_fixture(fixture_case):
    """The vote gives 1.228 with 614 of the 1133 joint inliers; under the stored
    solver ratio, 22.82, not one of them transfers.  Float32 against float64:
    the same voters, and every voter's count differs by at most the number of
    tested edgels within 0.01 px of the gate under that voter's float64 scale."""
    import scale_reference as SR
    c = fixture_case
    r32 = SR.fit(c["sel"], c["loc"], c["K"], scale_in=c["ratio"])
    r64 = SR.fit64(c["sel"], c["loc"], c["K"])
    print(f"noisy fixture: float32 {r32['scale31']!r} {r32['transfer_inliers']} of {r32['tested']} (voter "
          f"{r32['voter']}), float64 {r64['scale31']!r} {r64['transfer_inliers']} (voter {r64['voter']}); "
          f"largest count difference {np.abs(r32['counts'] - r64['counts']).max()}, near the gate at most "
          f"{r64['near'].max()}")
    assert abs(c["ratio"] - 22.82) < 0.01
    assert r32["joint"] == 1133 and r32["status"] == 0
    assert (r32["transfer_inliers"], r32["voter"]) == (614, 5039) and abs(float(r32["scale31"]) - 1.228) < 5e-4
    assert np.array_equal(r32["voters"], r64["voters"]) and r32["tested"] == r64["tested"]
    assert (np.abs(r32["counts"] - r64["counts"]) <= r64["near"]).all()
    assert abs(r32["transfer_inliers"] - r64["transfer_inliers"]) <= int(r64["near"].max())
    m21, m31 = RR.score(c["loc"], c["K"], tuple(np.asarray(c["sel"][k], np.float32) for k in RR.POSE_KEYS))
    assert int(r32["mask"].sum()) == r32["transfer_inliers"] and not r32["mask"][~(m21 & m31)].any()
    # under the solver's own ratio nothing transfers
    P = SR._pose(c["sel"], np.float32)
    _, Y, _, p = SR._edgels(c["loc"], c["K"], P, np.float32)
    idx = r32["tested_idx"]
    Z2, err = SR._error(tuple(y[idx] for y in Y), tuple(x[idx] for x in p), np.float32(c["ratio"]), P[3], c["K"],
                        np.float32)
    assert int(((Z2 > 0) & (err < 2)).sum()) == 0


def test_reference_without_a_voter(ransac0):
    import scale_reference as SR
    gt = RR.gt_pose(ransac0)
    r = SR.fit(gt, ransac0.locations[:65], ransac0.K, scale_in=3.5, has_path=False)
    assert r["status"] == SR.NONE and float(r["scale31"]) == 3.5 and not r["mask"].any()
    far = np.array(ransac0.locations[:65])
    far[:, 4:6] += 0.5                                   # view 3 far off: no joint inlier
    r = SR.fit(gt, far, ransac0.K, scale_in=3.5)
    assert (r["status"], r["joint"], r["tested"], r["num_voters"]) == (SR.NO_VOTER, 0, 0, 0)
    assert float(r["scale31"]) == 3.5 and r["voter"] == -1 and r["transfer_inliers"] == 0
    words = [sum(1 << b for b in range(64) if 64 * w + b < 130 and (64 * w + b) % 3 == 0) for w in range(3)]
    assert SR.pack(np.arange(130) % 3 == 0).tolist() == words and words[2] == 0b10
