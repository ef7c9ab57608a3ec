"""CPU tests of the three-view refinement's host side
(include/threeview/hc_pose_threeview.h): the struct layouts and macro values
through the C compiler, the header declaring no function, the mode switch on
hcRefineSettings::pad with its argument checks made before any device work, the
Python wrappers' own checks, and the numpy reference of the rule
(tests/threeview_reference.py) on the config-5 fixture, on the eight refined
candidates of trial 12 and on the noiseless scene.

The reference's figures (float32 counting, everything else float64; printed by
test_reference_figures), transfer inliers | rot21 | rot31 | t21 | t31 (rad) |
relative scale error, before -> after, and the best iterate:
  fixture winner  2664 -> 2713 | 0.00295 -> 0.00047 | 0.00603 -> 0.00054 | 0.00131 -> <1e-5   | 0.00294 -> 0.00019 | 5.6e-4 -> 5e-5 | 7
  trial 12 rank 2 2603 -> 2692 | 0.01464 -> 0.00151 | 0.00500 -> 0.00149 | 0.00778 -> 0.00077 | 0.00235 -> 0.00058 | 5.0e-3 -> 4e-5 | 4
  trial 12 rank 4 2649 -> 2694 | 0.01455 -> 0.00164 | 0.00202 -> 0.00146 | 0.00742 -> 0.00085 | 0.00071 -> 0.00054 | 4.5e-3 -> 1e-5 | 4
  trial 12 rank 6 2652 -> 2690 | 0.01605 -> 0.00134 | 0.00175 -> 0.00138 | 0.00796 -> 0.00057 | 0.00081 -> 0.00053 | 4.6e-3 -> 1.1e-4 | 3
The sum of the two rotation residuals falls by factors of 9.0, 6.6, 5.4 and 6.5.
The wrong-basin ranks 0, 1, 3, 5, 7 end with 693, 33, 713, 261 and 131 transfer
inliers (joint 1153, 605, 1186, 498, 291)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import refine_reference as RR
from checks import NOISE_SEED, golden, noisy_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "threeview", "hc_pose_threeview.h")
INVALID = 1
TRUE_SCALE = 1.1852790          # dataset 000, tests/test_scale31_host.py
REFINE_CALLS = ("hc_trifocal_pose_refine", "hc_trifocal_pose_refine_grouped", "hc_trifocal_pose_refine_topk",
                "hc_trifocal_pose_refine_topk_grouped")
RIGHT, WRONG = (2, 4, 6), (0, 1, 3, 5, 7)    # trial 12's ranks by basin (tests/test_gpu_scale31.py)


# ---- the ABI of the header ------------------------------------------------------------------

def test_header_declares_structs_and_macros_only():
    """No prototype, no stream: the stage is a mode of the refine calls, so the
    sets of entry points that the other host tests pin do not change."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"\b(hc_\w+)\s*\(", src) == []
    assert "hcStream" not in src and "hcStatus" not in src
    assert set(re.findall(r"\}\s*(\w+)\s*;", src)) == {"hcThreeViewReport", "hcRefineThreeViewSettings"}
    assert set(re.findall(r"#define\s+(HC_\w+)", src)) - {"HC_POSE_THREEVIEW_H"} == set(_abi.THREEVIEW_CONSTANTS)
    # additive: no struct of the other headers changed, and no symbol was added for it
    assert _abi.lib().hc_trifocal_abi_version() == _abi.ABI_VERSION == 2
    assert (C.sizeof(_abi.hcRefineSettings), C.sizeof(_abi.hcRefineReport), C.sizeof(_abi.hcTrifocalSelection),
            C.sizeof(_abi.hcScaleReport), C.sizeof(_abi.hcRefineScaleSettings)) == (16, 176, 136, 40, 32)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert not [ln for ln in exported.splitlines() if "threeview" in ln.lower() or "refine3" in ln.lower()]


def test_struct_mirrors_and_constants_match_the_header_by_the_c_compiler(tmp_path):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    structs = (_abi.hcThreeViewReport, _abi.hcRefineThreeViewSettings)
    names = sorted(_abi.THREEVIEW_CONSTANTS)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "threeview/hc_pose_threeview.h"', 'int main(void) {',
             '    hcRefineThreeViewSettings s; const hcRefineSettings *h = (const hcRefineSettings *)&s;']
    for s in structs:
        args = "".join(f", offsetof({s.__name__}, {f[0]})" for f in s._fields_)
        lines.append(f'    printf("{"%zu " * (1 + len(s._fields_))}\\n", sizeof({s.__name__}){args});')
    lines += [f'    printf("{"%ld " * len(names)}%d\\n", {", ".join(f"(long){n}" for n in names)}, '
              '(const void *)h == (const void *)&s.head);', '    return 0;', '}', '']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    for s, line in zip(structs, out):
        got = [int(v) for v in line.split()]
        assert got == [C.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_], s.__name__
    assert (C.sizeof(_abi.hcThreeViewReport), C.sizeof(_abi.hcRefineThreeViewSettings)) == (328, 48)
    assert _abi.THREEVIEW_REPORT_BYTES == 328 and _abi.hcThreeViewReport.rms_px_in.offset == 296
    assert _abi.hcRefineThreeViewSettings.head.offset == 0
    assert _abi.hcRefineThreeViewSettings._fields_[0][1] is _abi.hcRefineSettings
    assert [int(v) for v in out[2].split()] == [_abi.THREEVIEW_CONSTANTS[n] for n in names] + [1]
    assert _abi.HC_REFINE_THREEVIEW == int.from_bytes(b"TV31", "big") != _abi.HC_REFINE_SCALE31
    assert (_abi.HC_THREEVIEW_SELECT_BY_TRANSFER, _abi.HC_THREEVIEW_NONE, _abi.HC_THREEVIEW_TOO_FEW,
            _abi.HC_THREEVIEW_SINGULAR, _abi.HC_THREEVIEW_SKIPPED) == (2, 1, 2, 4, 8)


def _settings(bits=0, iterations=0, scale=0x2000, reports=0x4000, mask=None, iterations3=0, pad=0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    s = _abi.hcRefineThreeViewSettings()
    s.head.iterations = iterations
    s.head.pad[0] = _abi.HC_REFINE_THREEVIEW
    s.head.pad[1] = bits
    s.scale_reports, s.reports, s.transfer_mask = scale, reports, mask
    s.iterations3, s.pad = iterations3, pad
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
        bad = [_settings(scale=None), _settings(reports=None),                # NULL reports of either kind
               _settings(bits=1), _settings(bits=4), _settings(bits=-1), _settings(bits=1 << 30),   # undefined bits
               _settings(iterations3=33), _settings(iterations3=-1), _settings(pad=1),
               _settings(iterations=33), _settings(iterations=-1)]            # the head's own range still holds
        if not topk:
            bad.append(_settings(bits=_abi.HC_THREEVIEW_SELECT_BY_TRANSFER))  # the top-k calls only
        if not single:
            bad.append(_settings(mask=0x3000))                                # the single call only
        for s in bad:
            a = list(good)
            a[i] = C.cast(C.pointer(s), RS)
            assert getattr(L, name)(*a) == INVALID, (name, s.head.iterations, s.head.pad[1], s.scale_reports,
                                                     s.reports, s.transfer_mask, s.iterations3, s.pad)
        # the other arguments are still checked in the mode
        a = list(good)
        a[i] = C.cast(C.pointer(_settings()), RS)
        a[0] = None if isinstance(good[0], C.c_void_p) else 0
        assert getattr(L, name)(*a) == INVALID, name


def test_python_wrappers_reject_bad_keywords_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    bad = [dict(three_view=1), dict(three_view="yes"), dict(three_view_iterations=5),       # iterations need the mode
           dict(three_view=True, three_view_iterations=0), dict(three_view=True, three_view_iterations=33),
           dict(three_view=True, three_view_iterations=2.0), dict(three_view=True, three_view_iterations=True),
           dict(three_view=True, fit_scale=1), dict(three_view=True, transfer_mask=1)]
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
    with pytest.raises(_abi.HCError):
        pose.launch_refine_joint_grouped(None, None, three_view=True, transfer_mask=True)    # one scene only
    for kw in (dict(three_view=True, select_by_transfer=0), dict(three_view=True, transfer_mask=True)):
        with pytest.raises(_abi.HCError):
            pose.launch_refine_topk([None, None], None, None, **kw)
        with pytest.raises(_abi.HCError):
            pose.select_refined(None, None, None, None, **kw)
    with pytest.raises(TypeError):
        pose.launch_refine_joint(None, None, None, three_view=True, select_by_transfer=True)  # top-k only


def test_three_view_report_dict_decodes_the_struct():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    r = _abi.hcThreeViewReport()
    r.status, r.iterations_run, r.best_iteration, r.fit_set, r.transfer_inliers = 6, 4, 2, 3629, 2713
    r.transfer_history[:] = [2664, 2707, 2713, 100, 0] + [-1] * 28
    r.joint_history[:] = [3640, 3630, 3629, 200, 3] + [-1] * 28
    r.scale_in, r.scale_out = 1.25, 1.1875
    r.rms_px_in[:], r.rms_px_out[:] = [1.0, 1.75], [0.5, 1.5]
    d = pose.three_view_report_dict(np.frombuffer(bytes(r), np.uint8))
    assert (d["status"], d["none"], d["too_few"], d["singular"], d["skipped"]) == (6, False, True, True, False)
    assert (d["iterations_run"], d["best_iteration"], d["fit_set"], d["transfer_inliers"]) == (4, 2, 3629, 2713)
    assert d["transfer_history"][:6].tolist() == [2664, 2707, 2713, 100, 0, -1] and d["joint_history"][2] == 3629
    assert (float(d["scale_in"]), float(d["scale_out"])) == (1.25, 1.1875)
    assert d["rms_px_in"].tolist() == [1.0, 1.75] and d["rms_px_out"].tolist() == [0.5, 1.5]
    r.status = _abi.HC_THREEVIEW_SKIPPED | _abi.HC_THREEVIEW_NONE
    d = pose.three_view_report_dict(np.frombuffer(bytes(r), np.uint8))
    assert d["skipped"] and d["none"] and not d["too_few"]


# ---- the reference -------------------------------------------------------------------------------

def _angle(Rg, R):
    M = np.asarray(Rg, np.float64).reshape(3, 3).T @ np.asarray(R, np.float64).reshape(3, 3)
    return float(np.arccos(np.clip(0.5 * (np.trace(M) - 1.0), -1.0, 1.0)))


def _tilt(tg, t):
    tg = np.asarray(tg, np.float64)
    return float(np.arccos(np.clip((tg / np.linalg.norm(tg)) @ np.asarray(t, np.float64), -1.0, 1.0)))


def _errors(data, d):
    """(rot21, rot31, t21 angle, t31 angle) in rad and the scale's relative error against the GT."""
    return (_angle(data.pose21[:9], d["R21"]), _angle(data.pose31[:9], d["R31"]), _tilt(data.pose21[9:], d["t21"]),
            _tilt(data.pose31[9:], d["t31"]), abs(float(d["scale31"]) - TRUE_SCALE) / TRUE_SCALE)


def stage2(pose24, counts, loc, K):
    """The selection stages 1 and 2 produce from a two-view-refined pose: its
    24 floats, its counts, and the voted scale (scale_reference.fit)."""
    import scale_reference as SR
    sel = dict(R21=pose24[0:9], t21=pose24[9:12], R31=pose24[12:21], t31=pose24[21:24], inliers=int(counts[0]),
               inliers21=int(counts[1]), inliers31=int(counts[2]))
    vote = SR.fit(sel, loc, K)
    sel["scale31"] = vote["scale31"]
    return sel, vote


@pytest.fixture(scope="module")
def cases(oracle, ransac0):
    """name -> (stage 2's selection, its vote, the reference's result): the
    fixture's joint winner and trial 12's eight candidates, each two-view
    refined by refine_reference.refine (trial 12: the committed record of it)."""
    import threeview_reference as TV
    out = {}
    g = golden("pose_joint_noisy1px_N100")
    loc = oracle.add_pixel_noise(ransac0.locations, ransac0.K, 1.0, NOISE_SEED)
    i = int(np.nonzero(g["cand_ids"] == g["path"])[0][0])
    _, sel = oracle.pose_support(g["cand_tracks"][i:i + 1], np.ones(1, np.uint8), loc, ransac0.K)
    r = RR.refine(sel, loc, ransac0.K)
    p24 = np.concatenate([r[k].reshape(-1) for k in RR.POSE_KEYS])
    s2, vote = stage2(p24, (r["inliers"], r["inliers21"], r["inliers31"]), loc, ransac0.K)
    out["fixture"] = (s2, vote, TV.refine3(s2, loc, ransac0.K))
    g = golden("pose_topk_noisy1px_trial12_N100")
    loc = noisy_data(NOISE_SEED + 12).locations
    for rank in range(8):
        s2, vote = stage2(g["ref_pose"][rank], g["ref_counts"][rank], loc, ransac0.K)
        out[rank] = (s2, vote, TV.refine3(s2, loc, ransac0.K))
    return out


def test_reference_figures(cases, ransac0):
    """Prints the before and after figures of all nine cases; on the four
    right-basin cases the sum of the two rotation residuals falls to at most a
    third, and both translation angles and the scale error fall."""
    for name, (s2, vote, r) in cases.items():
        b, a = _errors(ransac0, s2), _errors(ransac0, r)
        print(f"{name}: transfer {vote['transfer_inliers']} -> {r['transfer_inliers']} of |F| {r['fit_set']}, joint "
              f"{s2['inliers']} -> {r['inliers']}, best {r['best_iteration']}, status {r['status']}, history "
              f"{r['transfer_history'][:r['iterations_run'] + 1].tolist()}\n    rot21 {b[0]:.5f} -> {a[0]:.5f}, rot31 "
              f"{b[1]:.5f} -> {a[1]:.5f}, t21 {b[2]:.5f} -> {a[2]:.5f}, t31 {b[3]:.5f} -> {a[3]:.5f}, scale "
              f"{b[4]:.2e} -> {a[4]:.2e}, rotation sum x {(b[0] + b[1]) / (a[0] + a[1]):.2f}, rms "
              f"{r['rms_px_in'].tolist()} -> {r['rms_px_out'].tolist()}")
        assert vote["transfer_inliers"] == r["transfer_history"][0] and r["transfer_inliers"] == r["transfer_history"].max()
    for name in ("fixture",) + RIGHT:
        s2, vote, r = cases[name]
        b, a = _errors(ransac0, s2), _errors(ransac0, r)
        assert a[0] + a[1] <= (b[0] + b[1]) / 3.0, name
        assert a[2] < b[2] and a[3] < b[3] and a[4] < b[4], name
        assert r["status"] == 0 and r["best_iteration"] > 0 and r["transfer_inliers"] > vote["transfer_inliers"], name
        assert r["transfer_inliers"] >= 2690 and r["inliers"] >= 3629, name


def test_reference_leaves_the_wrong_basin_separable(cases):
    for rank in WRONG:
        assert cases[rank][2]["transfer_inliers"] < 1000, rank
    assert min(cases[n][2]["transfer_inliers"] for n in ("fixture",) + RIGHT) >= 2690


def test_reference_returns_rank_1_bit_for_bit(cases):
    """Rank 1's first step leaves it without a fit set: history 33, 0."""
    import threeview_reference as TV
    s2, vote, r = cases[1]
    assert r["best_iteration"] == 0 and r["status"] == TV.TOO_FEW and r["iterations_run"] == 1
    assert r["transfer_history"][:3].tolist() == [33, 0, -1]
    for k in RR.POSE_KEYS:
        assert r[k].tobytes() == np.asarray(s2[k], np.float32).tobytes(), k
    assert np.float32(r["scale31"]).tobytes() == np.float32(s2["scale31"]).tobytes()
    assert (r["inliers"], r["inliers21"], r["inliers31"]) == (s2["inliers"], s2["inliers21"], s2["inliers31"])


def test_reference_on_the_noiseless_scene(ransac0):
    """257 clean edgels, the GT turned by 3e-4 rad: every iterate keeps 257 of
    257 and the scale ends within 1e-5 of the truth."""
    import threeview_reference as TV
    loc = ransac0.locations[:257]
    p = RR.perturbed(RR.gt_pose(ransac0))
    m21, m31 = RR.score(loc, ransac0.K, tuple(p[k] for k in RR.POSE_KEYS))
    p24 = np.concatenate([p[k].reshape(-1) for k in RR.POSE_KEYS])
    s2, vote = stage2(p24, (int((m21 & m31).sum()), int(m21.sum()), int(m31.sum())), loc, ransac0.K)
    r = TV.refine3(s2, loc, ransac0.K)
    print(f"clean 257: scale {s2['scale31']!r} -> {r['scale31']!r}, history {r['transfer_history'][:11].tolist()}")
    assert r["status"] == 0 and r["iterations_run"] == 10
    assert (r["transfer_history"][:11] == 257).all() and (r["joint_history"][:11] == 257).all() and r["fit_set"] == 257
    assert abs(float(r["scale31"]) - TRUE_SCALE) < 1e-5
    assert (r["rms_px_out"] < 1e-3).all() and (r["rms_px_in"] > 0.1).all()
