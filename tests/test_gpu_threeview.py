"""GPU tests of the three-view refinement (include/threeview/hc_pose_threeview.h),
the third stage of the four refine calls.  The device's stage is compared with
the numpy reference (tests/threeview_reference.py) started from the device's own
stage-2 output, the selection a fit_scale call returns, so a difference is the
stage's alone.

Scenes: "noisy", the config-5 fixture (the joint winner of
pose_joint_noisy1px_N100.npz on the 5117 edgels with 1 px noise); the eight
candidates of trial 12 (pose_topk_noisy1px_trial12_N100.npz); "clean", the
noiseless edgels of dataset 000 under the GT pose turned by 3e-4 rad, cut to the
sizes either side of min_inliers (16), of the wave (64) and of the workgroup's
256 threads, and whole (5117: twenty edgels per thread).

Bounds (the project's own, tests/test_gpu_refine.py): the 24 pose floats and
scale31 within ten float32 steps at 1 (6e-7) of the reference's iterate; every
count and history entry within the number of edgels that lie within 0.01 px of
a 2 px gate (view 2, view 3 or the transfer) under the reference's state at that
iterate; the best iterations equal unless the reference's two entries tie within
that allowance.
"""
import ctypes as C

import numpy as np
import pytest

import graph_common as G
import refine_reference as RR
import scale_reference as SR
import threeview_reference as TV
from checks import NOISE_SEED, golden, noisy_data
from refine_reference import POSE_KEYS, gt_pose, perturbed

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 257, 5117]
TRUE_SCALE = 1.1852790          # dataset 000, tests/test_scale31_host.py
POSE_BOUND = 10 * 2.0 ** -24    # 6e-7
# Largest differences to the reference measured on an MI355X over every compared
# selection of this file (printed by _compare): the pose floats, scale31, and a
# count or history entry against its allowance.
MEASURED_D = 6.664e-08      # trial 12's rank 7 (one float of R21 a step off); 0 on the 19 other selections
MEASURED_SCALE = 0.0        # every scale31 is the reference's bits
MEASURED_COUNT = 0          # every count and history entry is the reference's, where up to 75 edgels lie near a gate
COUNT_KEYS = ("inliers", "inliers21", "inliers31", "fit_set", "transfer_inliers")


def _popcount(words):
    return sum(bin(int(v)).count("1") for v in words)


def _selection(pose32, loc, K, path=23612, num_candidates=31, scale31=1.75):
    """A joint selection of the given pose with the counts it has on the scene."""
    m21, m31 = RR.score(loc, K, tuple(pose32[k] for k in POSE_KEYS))
    cJ = int((m21 & m31).sum())
    d = dict(num_candidates=num_candidates, path=path, inliers=cJ, inliers21=int(m21.sum()),
             inliers31=int(m31.sum()), key=(cJ << 32) | path, scale31=np.float32(scale31))
    d.update({k: np.asarray(pose32[k], np.float32) for k in POSE_KEYS})
    return d


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _upload(sel, dev):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    return _dev(np.frombuffer(bytes(pose.joint_selection_from_dict(sel)), np.uint8).copy(), dev)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _struct_bytes(sel):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    return bytes(pose.joint_selection_from_dict(sel))


def _compare(what, out, tv, stage2, loc, K, iterations=10, min_inliers=16, mask=None):
    """A device result (selection dict, three-view report dict) against the
    reference run from stage2, the selection dict the stage started from."""
    ref = TV.refine3(stage2, loc, K, iterations, min_inliers)
    n = ref["iterations_run"] + 1
    near = ref["near"]
    bk, rk = tv["best_iteration"], ref["best_iteration"]
    print(f"{what}: transfer {tv['transfer_history'][:n].tolist()} | {ref['transfer_history'][:n].tolist()}, joint "
          f"{tv['joint_history'][:n].tolist()} | {ref['joint_history'][:n].tolist()}, near {near[:n].tolist()}, best "
          f"{bk} | {rk}, status {tv['status']} | {ref['status']}, scale {tv['scale_in']!r} -> {tv['scale_out']!r} | "
          f"{ref['scale31']!r}, rms {tv['rms_px_in'].tolist()} -> {tv['rms_px_out'].tolist()} | "
          f"{ref['rms_px_out'].tolist()}")
    assert (tv["status"], tv["iterations_run"]) == (ref["status"], ref["iterations_run"]), what
    assert not tv["skipped"] and not tv["none"]
    for name in ("transfer_history", "joint_history"):
        h, r = tv[name].astype(np.int64), ref[name].astype(np.int64)
        assert (h[n:] == -1).all() and (np.abs(h[:n] - r[:n]) <= near[:n]).all(), (what, name)
    if bk != rk:            # only where the reference's two entries tie within the allowance
        assert abs(int(ref["transfer_history"][bk]) - int(ref["transfer_history"][rk])) <= near[bk] + near[rk], what
    it = ref["iterates"][bk]
    d = RR.pose_distance(out, it)
    ds = abs(float(out["scale31"]) - float(it["scale31"]))
    dc = max(abs(int(tv[k] if k in tv else out[k]) - int(it[k])) for k in COUNT_KEYS) if bk > 0 else 0
    print(f"    d = {d:.3e}, scale difference {ds:.3e}, largest count difference {dc} (allowance {near[bk]})")
    assert d <= POSE_BOUND and ds <= POSE_BOUND and MEASURED_D <= POSE_BOUND, what
    assert tv["scale_out"].tobytes() == out["scale31"].tobytes() and tv["scale_in"].tobytes() == \
        np.float32(stage2["scale31"]).tobytes(), what
    assert tv["transfer_inliers"] == tv["transfer_history"][bk] == tv["transfer_history"].max(), what
    if bk == 0:             # the values it came in with, bit for bit
        assert _struct_bytes(out) == _struct_bytes(stage2), what
    else:
        assert dc <= near[bk], what
        assert out["inliers"] == tv["joint_history"][bk] and out["key"] == (out["inliers"] << 32) | out["path"], what
        assert (out["path"], out["num_candidates"]) == (stage2["path"], stage2["num_candidates"]), what
    assert np.abs(tv["rms_px_in"] - ref["rms_px_in"]).max() < 1e-9, what      # iterate 0: the same set, summed otherwise
    if near[bk] == 0:
        assert np.abs(tv["rms_px_out"] - it["rms_px"]).max() < 1e-6, what
    if mask is not None:
        assert _popcount(mask) == tv["transfer_inliers"], what
        if near[bk] == 0 and d == 0.0 and ds == 0.0:
            assert np.array_equal(mask, SR.pack(it["mask"])), what
    return ref


@pytest.fixture(scope="module")
def scenes(tracker, ransac0):
    """Per scene kind: the host edgels, their device copy, K and the input pose."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = tracker.device
    noisy0 = noisy_data()
    g = golden("pose_joint_noisy1px_N100")
    i = int(np.nonzero(g["cand_ids"] == g["path"])[0][0])
    tr = np.zeros((312, 31, 2), np.float32)
    tr[:, 30, 0] = 1.0
    tr[5] = g["cand_tracks"][i]
    conv = np.zeros(312, np.uint8)
    conv[5] = 1
    K = _dev(noisy0.K, dev)
    noisy_dev = _dev(np.array(noisy0.locations), dev)
    _, winner = pose.pose_support_joint(_dev(tr, dev), _dev(conv, dev), noisy_dev, K)
    assert [winner["inliers"], winner["inliers21"], winner["inliers31"]] == g["inliers"].tolist()
    assert np.array_equal(noisy0.K, ransac0.K)
    return {"noisy": dict(loc=noisy0.locations, dev=noisy_dev, K=noisy0.K, Kdev=K, pose=winner, data=noisy0),
            "clean": dict(loc=ransac0.locations, dev=_dev(np.array(ransac0.locations), dev), K=ransac0.K, Kdev=K,
                          pose=perturbed(gt_pose(ransac0)), data=ransac0)}


def _case(scenes, kind, E, **kw):
    s = scenes[kind]
    return _selection(s["pose"], s["loc"][:E], s["K"], **kw), s["dev"][:E], s["Kdev"], s["loc"][:E]


# ---- the fixture ------------------------------------------------------------------------------------

def test_noisy_fixture_against_the_reference(scenes):
    """Stages 1 and 2 are the fit_scale call's, bit for bit; stage 3 raises the
    transfer support and brings both rotations within 1e-3 rad of the GT."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    s = scenes["noisy"]
    sel, edgels, K = s["pose"], s["dev"], s["Kdev"]
    in_dev = _upload(sel, edgels.device)
    two_dev, report2, scale2, _ = pose.launch_refine_joint(in_dev, edgels, K, fit_scale=True)
    two = pose.joint_selection_dict(pose.joint_selection_struct(two_dev))
    _, report, scale, _, _ = pose.launch_refine_joint(in_dev, edgels, K, three_view=True)
    assert _bytes(report) == _bytes(report2) and _bytes(scale) == _bytes(scale2)
    out, rep, out_dev = pose.refine_joint(in_dev, edgels, K, three_view=True, transfer_mask=True,
                                          return_device_selection=True)
    tv = rep["three_view"]
    assert rep["scale"] == pose.scale_report_dict(scale2)
    assert tv["transfer_history"][0] == rep["scale"]["transfer_inliers"] and tv["joint_history"][0] == two["inliers"]
    ref = _compare("noisy fixture", out, tv, two, s["loc"], s["K"], mask=tv["mask"])
    assert tv["status"] == 0 and tv["best_iteration"] > 0 and tv["transfer_inliers"] > rep["scale"]["transfer_inliers"]
    assert ref["transfer_inliers"] >= 2700
    joint = pose.inlier_mask(out_dev, edgels, K, packed=True)
    assert _popcount(joint) == out["inliers"] and not (tv["mask"] & ~joint).any()
    before, _ = pose.residuals(s["data"], two)
    after, ok = pose.residuals(s["data"], out)
    print(f"    residuals {before.tolist()} -> {after.tolist()}, scale {two['scale31']!r} -> {out['scale31']!r}")
    assert ok and after[0] + after[1] <= (before[0] + before[1]) / 3.0 and max(after[0], after[1]) < 1e-3
    assert abs(float(out["scale31"]) - TRUE_SCALE) < abs(float(two["scale31"]) - TRUE_SCALE) < 0.02
    # fewer steps are a prefix
    _, rep3 = pose.refine_joint(in_dev, edgels, K, three_view=True, three_view_iterations=3)
    t3 = rep3["three_view"]
    assert t3["iterations_run"] == 3 and t3["transfer_history"][:4].tolist() == tv["transfer_history"][:4].tolist()
    assert (t3["transfer_history"][4:] == -1).all() and t3["transfer_inliers"] == t3["transfer_history"][:4].max()


# ---- trial 12: the eight candidates through the top-k call -----------------------------------------

@pytest.fixture(scope="module")
def trial12(tracker):
    """The run's candidates at their batch ids of a 31 200-path launch, scored
    on the 5117 noisy edgels by the joint call, and its 8 best."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = tracker.device
    g = golden("pose_topk_noisy1px_trial12_N100")
    data = noisy_data(NOISE_SEED + 12)
    ids = g["cand_ids"]
    tr = np.zeros((31200, 31, 2), np.float32)
    tr[:, 30, 0] = 1.0
    tr[ids] = g["cand_tracks"]
    conv = np.zeros(31200, np.uint8)
    conv[ids] = 1
    edgels, K = _dev(np.array(data.locations), dev), _dev(data.K, dev)
    T, Cv = _dev(tr, dev), _dev(conv, dev)
    inl = torch.empty((31200, 3), dtype=torch.int32, device=dev)
    sel = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    pose.launch_pose_support_joint(T, Cv, edgels, K, inl, sel)
    cand = pose.launch_topk_joint(T, inl, 8)
    torch.cuda.synchronize(dev)
    return dict(data=data, edgels=edgels, K=K, tracks=T, conv=Cv, cand=cand)


def test_trial12_topk_with_and_without_selection_by_transfer(trial12):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    c = trial12
    _, _, two, rep2 = pose.refine_topk(c["cand"], c["edgels"], c["K"], fit_scale=True)
    bj, rj, rd, pd = pose.refine_topk(c["cand"], c["edgels"], c["K"], three_view=True)
    bt, rt, rdt, pdt = pose.refine_topk(c["cand"], c["edgels"], c["K"], three_view=True, select_by_transfer=True)
    assert [_struct_bytes(d) for d in rd] == [_struct_bytes(d) for d in rdt]
    tkeys, jkeys = [], []
    for r in range(8):
        assert pd[r]["scale"] == rep2[r]["scale"], r
        ref = _compare(f"trial 12 rank {r}", rd[r], pd[r]["three_view"], two[r], c["data"].locations, c["data"].K)
        tkeys.append((pd[r]["three_view"]["transfer_inliers"] << 32) | rd[r]["path"])
        jkeys.append(rd[r]["key"])
        if r in (2, 4, 6):
            assert ref["transfer_inliers"] >= 2690 and pd[r]["three_view"]["best_iteration"] > 0, r
            res, ok = pose.residuals(c["data"], rd[r])
            assert ok and max(res[0], res[1]) < 3e-3 and abs(float(rd[r]["scale31"]) - TRUE_SCALE) < 1e-3, r
        else:
            assert ref["transfer_inliers"] < 1000, r
    # rank 1's first step leaves it without a fit set: it comes back as stage 2 left it
    assert pd[1]["three_view"]["best_iteration"] == 0 and pd[1]["three_view"]["too_few"]
    assert _struct_bytes(rd[1]) == _struct_bytes(two[1])
    # the selection is the rule's on the device's own keys
    assert rj == int(np.argmax(jkeys)) and _struct_bytes(bj) == _struct_bytes(rd[rj]) and rj in (2, 4, 6)
    assert rt == int(np.argmax(tkeys)) and _struct_bytes(bt) == _struct_bytes(rd[rt]) and rt in (2, 4, 6)
    # the whole chain on one stream
    b2, info = pose.select_refined(c["tracks"], c["conv"], c["edgels"], c["K"], k=8, three_view=True,
                                   select_by_transfer=True)
    assert _struct_bytes(b2) == _struct_bytes(bt) and info["best_rank"] == rt
    assert info["three_view"]["transfer_inliers"] == tkeys[rt] >> 32


# ---- clean scenes at the sizes where the kernel changes path ------------------------------------------

@pytest.mark.parametrize("E", SIZES)
def test_clean_scenes_against_the_reference(scenes, E):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, K, loc = _case(scenes, "clean", E)
    in_dev = _upload(sel, edgels.device)
    keep = _bytes(in_dev)
    two_dev, _, _, _ = pose.launch_refine_joint(in_dev, edgels, K, fit_scale=True)
    two = pose.joint_selection_dict(pose.joint_selection_struct(two_dev))
    out, rep, out_dev = pose.refine_joint(in_dev, edgels, K, three_view=True, transfer_mask=True,
                                          return_device_selection=True)
    tv = rep["three_view"]
    assert _bytes(in_dev) == keep and sel["inliers"] == E        # under a pixel off: every edgel is a joint inlier
    _compare(f"clean E={E}", out, tv, two, loc, scenes["clean"]["K"], mask=tv["mask"])
    assert len(tv["mask"]) == (E + 63) // 64
    if E < 16:
        assert tv["status"] == TV.TOO_FEW and tv["too_few"] and tv["iterations_run"] == tv["best_iteration"] == 0
        assert _bytes(out_dev) == _bytes(two_dev) and tv["fit_set"] == E == tv["transfer_inliers"]
        assert (tv["transfer_history"][1:] == -1).all()
    else:
        assert tv["status"] == 0 and tv["iterations_run"] == 10
        assert (tv["transfer_history"][:11] == E).all() and (tv["joint_history"][:11] == E).all()
        assert tv["fit_set"] == E == out["inliers"] and _popcount(tv["mask"]) == E
        assert (tv["rms_px_out"] < 1e-3).all()             # noiseless: the fit is exact (stage 1 already is, in view 2)
        assert abs(float(out["scale31"]) - TRUE_SCALE) < (1e-5 if E >= 257 else 1e-3)
    # out == in is allowed, and a second call gives the same bytes
    alias = in_dev.clone()
    o2, _, _, w2, t2 = pose.launch_refine_joint(alias, edgels, K, out=alias, three_view=True, transfer_mask=True)
    assert o2.data_ptr() == alias.data_ptr() and _bytes(alias) == _bytes(out_dev)
    assert pose.three_view_report_dict(t2)["transfer_history"].tolist() == tv["transfer_history"].tolist()
    assert np.array_equal(w2.cpu().numpy().view(np.uint64), tv["mask"])


# ---- the stage skipped -----------------------------------------------------------------------------

def test_no_path_and_no_voter_skip_the_stage(scenes, ransac0):
    """Without a path, and on the scale tests' scene without a voter (view 3
    moved far off), the output is stage 2's and the report says so."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    dev = scenes["clean"]["dev"].device
    Kd, K = scenes["clean"]["Kdev"], ransac0.K
    none = pose.joint_selection_dict(_abi.hcTrifocalSelection())
    none.update(path=-1, inliers=-1, inliers21=-1, inliers31=-1, scale31=np.float32(0.0))
    far = np.array(ransac0.locations[:65])
    far[:, 4:6] += 0.5
    sel = _selection(scenes["clean"]["pose"], far, K, scale31=3.5)
    assert SR.fit(sel, far, K, scale_in=3.5)["status"] == SR.NO_VOTER
    for name, s, edgels, status in (("none", none, scenes["clean"]["dev"][:257], 9), ("far", sel, _dev(far, dev), 8)):
        in_dev = _upload(s, dev)
        two_dev, rep2, scale2, _ = pose.launch_refine_joint(in_dev, edgels, Kd, fit_scale=True)
        out_dev, rep, scale, words, tvd = pose.launch_refine_joint(in_dev, edgels, Kd, three_view=True,
                                                                   transfer_mask=True)
        tv = pose.three_view_report_dict(tvd)
        assert _bytes(out_dev) == _bytes(two_dev) and _bytes(rep) == _bytes(rep2) and _bytes(scale) == _bytes(scale2), name
        assert tv["status"] == status and tv["skipped"] and tv["none"] == (name == "none"), name
        assert (tv["transfer_history"] == -1).all() and (tv["joint_history"] == -1).all(), name
        assert (tv["iterations_run"], tv["best_iteration"], tv["fit_set"], tv["transfer_inliers"]) == (0, 0, 0, 0), name
        assert float(tv["scale_in"]) == float(tv["scale_out"]) == float(s["scale31"]), name
        assert not tv["rms_px_in"].any() and not tv["rms_px_out"].any() and not words.cpu().numpy().any(), name
    assert pose.scale_report_dict(scale)["status"] == _abi.HC_SCALE_NO_VOTER
    # the top-k call with only such candidates: no best by either rule's keys but the path's own
    for kw in (dict(), dict(select_by_transfer=True)):
        best, rank, _, reps = pose.refine_topk([none, none], scenes["clean"]["dev"][:257], Kd, three_view=True, **kw)
        assert rank == -1 and best["path"] == -1 and all(r["three_view"]["skipped"] for r in reps)


def test_identical_edgels_without_a_derivative_are_singular(scenes, ransac0):
    """64 copies of one edgel under intrinsics whose focal lengths are 0: every
    pixel residual and every derivative is exactly 0, the first pivot is 0, and
    the stage ends with SINGULAR at iterate 0 and returns the best iterate so
    far, its input.  (With the data's own intrinsics the 1e-9 diag A term makes
    the rank-4 system of 64 identical edgels positive definite: the reference
    then runs to its end without the status.)"""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = scenes["clean"]["dev"].device
    loc = np.repeat(np.array(ransac0.locations[:1]), 64, axis=0)
    K = np.array(ransac0.K, np.float32)
    K[0] = K[4] = 0.0
    sel = _selection(scenes["clean"]["pose"], loc, K)
    assert sel["inliers"] == 64
    edgels, Kd = _dev(loc, dev), _dev(K, dev)
    in_dev = _upload(sel, dev)
    two_dev, _, _, _ = pose.launch_refine_joint(in_dev, edgels, Kd, fit_scale=True)
    two = pose.joint_selection_dict(pose.joint_selection_struct(two_dev))
    out, rep, out_dev = pose.refine_joint(in_dev, edgels, Kd, three_view=True, transfer_mask=True,
                                          return_device_selection=True)
    tv = rep["three_view"]
    ref = _compare("identical 64", out, tv, two, loc, K, mask=tv["mask"])
    assert ref["status"] == TV.SINGULAR and tv["singular"] and tv["status"] == TV.SINGULAR
    assert tv["iterations_run"] == tv["best_iteration"] == 0 and tv["transfer_history"][:2].tolist() == [64, -1]
    assert _bytes(out_dev) == _bytes(two_dev) and tv["fit_set"] == 64 and _popcount(tv["mask"]) == 64


# ---- grouped ----------------------------------------------------------------------------------------

def test_grouped_equals_single_calls(problem, scenes):
    """Four triplets of different E in one launch, 17, 65 and 129 (one, two and
    three of the four waves with an edgel; small scenes are the ill-conditioned
    ones) and 2049: every selection and report is the single call's on that
    triplet alone, bit for bit; the same through the grouped top-k call with
    two candidates per triplet."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    kinds = [("clean", 65), ("noisy", 2049), ("clean", 17), ("clean", 129)]
    batch = TripletBatch(problem, [scenes[k]["data"] for k, _ in kinds], seeds=0, samples_per_triplet=1,
                         edgel_counts=[E for _, E in kinds])
    cases = [_case(scenes, k, E, path=100 + i, num_candidates=3 + i) for i, (k, E) in enumerate(kinds)]
    dev = cases[0][1].device
    db = batch.to(dev)
    sels, reps, scales, tvs = pose.launch_refine_joint_grouped([c[0] for c in cases], db, three_view=True,
                                                               three_view_iterations=6)
    torch.cuda.synchronize(dev)
    S, R, Q, V = pose.JOINT_SEL_BYTES, pose.REPORT_BYTES, pose.SCALE_REPORT_BYTES, pose.THREEVIEW_REPORT_BYTES
    singles = []
    for t, (sel, edgels, K, loc) in enumerate(cases):
        one, rep, scale, _, tv = pose.launch_refine_joint(sel, edgels, K, three_view=True, three_view_iterations=6)
        assert _bytes(sels)[t * S:(t + 1) * S] == _bytes(one), t
        assert _bytes(reps)[t * R:(t + 1) * R] == _bytes(rep), t
        assert _bytes(scales)[t * Q:(t + 1) * Q] == _bytes(scale), t
        assert _bytes(tvs)[t * V:(t + 1) * V] == _bytes(tv), t
        d = pose.three_view_report_dict(tv)
        assert d["status"] == 0 and d["iterations_run"] == 6 and (d["transfer_history"][7:] == -1).all(), t
        singles.append((one, tv))
    assert pose.three_view_report_dict(singles[1][1])["best_iteration"] > 0      # the noisy triplet moves
    dicts, reports = pose.refine_joint_grouped([c[0] for c in cases], batch, device=dev, three_view=True,
                                               three_view_iterations=6)
    for t in range(4):
        assert _struct_bytes(dicts[t]) == _bytes(singles[t][0]), t
        assert reports[t]["three_view"]["transfer_history"].tolist() == \
            pose.three_view_report_dict(singles[t][1])["transfer_history"].tolist(), t
    # top-k, grouped: per triplet the selection itself and a second candidate ("none", or the same pose at another path)
    none = dict(cases[0][0], path=-1)
    cand = [cases[0][0], none, cases[1][0], dict(cases[1][0], path=7), cases[2][0], cases[2][0], cases[3][0], none]
    for kw in (dict(), dict(select_by_transfer=True)):
        out = pose.refine_topk_grouped(cand, db, 2, three_view=True, three_view_iterations=6, **kw)
        for t in range(4):
            assert _struct_bytes(out[t]["refined"][0]) == _bytes(singles[t][0]), t
            assert out[t]["reports"][0]["three_view"]["transfer_history"].tolist() == \
                pose.three_view_report_dict(singles[t][1])["transfer_history"].tolist(), t
        assert out[0]["reports"][1]["three_view"]["skipped"] and out[0]["best_rank"] == 0
        # equal counts: the larger path wins under both keys
        assert out[1]["best_rank"] == 0 and out[1]["best"]["path"] == 101
    with pytest.raises(Exception):
        pose.launch_refine_topk_grouped(cand, db, 2, three_view=True, transfer_mask=True)


# ---- graph capture and replay -------------------------------------------------------------------------

def test_graph_replay_of_the_three_stages(scenes):
    """launch_refine_joint(three_view=True) recorded once and replayed twice:
    both replays give the eager call's bytes, with every output poisoned from
    outside the graph before each replay."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, K, _ = _case(scenes, "noisy", 2049)
    in_dev = _upload(sel, edgels.device)

    def enqueue():
        return pose.launch_refine_joint(in_dev, edgels, K, three_view=True, transfer_mask=True)
    eager = [_bytes(t) for t in enqueue()]
    assert pose.three_view_report_dict(np.frombuffer(eager[4], np.uint8))["status"] == 0
    cap, out = G.capture(enqueue)
    try:
        for _ in range(2):
            G.poison(*out)
            cap.replay()
            torch.cuda.synchronize()
            assert [_bytes(t) for t in out] == eager
    finally:
        G.release(cap)


# ---- the mode off -------------------------------------------------------------------------------------

def test_mode_off_is_the_call_as_it_was(scenes, trial12):
    """On a selection whose best iterate is 0 (trial 12's rank 1) the mode's
    output is its stage 2's, the fit_scale call's, byte for byte, and the plain
    call's apart from scale31; zeroed settings and a pad the modes do not know
    give the plain call's bytes before and after a three-view call on the same
    buffers."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    c = trial12
    S = pose.JOINT_SEL_BYTES
    dev = c["edgels"].device
    in_dev = c["cand"][S:2 * S].clone()
    E = int(c["edgels"].shape[0])
    out = torch.empty(S, dtype=torch.uint8, device=dev)
    report = torch.empty(pose.REPORT_BYTES, dtype=torch.uint8, device=dev)

    def call(settings):
        G.poison(out, report)
        _abi.call("hc_trifocal_pose_refine", _abi.ptr(in_dev), E, _abi.ptr(c["edgels"]), _abi.ptr(c["K"]),
                  C.byref(settings) if settings is not None else None, _abi.ptr(out), _abi.ptr(report),
                  _abi.ptr(torch.cuda.current_stream(dev)))
        torch.cuda.synchronize(dev)
        return _bytes(out), _bytes(report)
    other = _abi.hcRefineSettings()
    other.pad[0], other.pad[1] = 0x54563330, 2            # one below the tag
    before = call(_abi.hcRefineSettings())
    assert call(None) == before and call(other) == before
    two, rep2, scale2, _ = pose.launch_refine_joint(in_dev, c["edgels"], c["K"], fit_scale=True)
    # a three-view call into the same buffers
    ts = _abi.hcRefineThreeViewSettings()
    ts.head.pad[0] = _abi.HC_REFINE_THREEVIEW
    scale = torch.empty(pose.SCALE_REPORT_BYTES, dtype=torch.uint8, device=dev)
    tvd = torch.empty(pose.THREEVIEW_REPORT_BYTES, dtype=torch.uint8, device=dev)
    ts.scale_reports, ts.reports = scale.data_ptr(), tvd.data_ptr()
    G.poison(out, report, scale, tvd)
    _abi.call("hc_trifocal_pose_refine", _abi.ptr(in_dev), E, _abi.ptr(c["edgels"]), _abi.ptr(c["K"]),
              C.cast(C.pointer(ts), C.POINTER(_abi.hcRefineSettings)), _abi.ptr(out), _abi.ptr(report),
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    tv = pose.three_view_report_dict(tvd)
    assert tv["best_iteration"] == 0 and tv["too_few"] and tv["iterations_run"] == 1
    assert _bytes(out) == _bytes(two) and _bytes(report) == _bytes(rep2) == before[1] and _bytes(scale) == _bytes(scale2)
    assert _bytes(out)[:128] == before[0][:128] and _bytes(out)[132:] == before[0][132:] and _bytes(out) != before[0]
    assert call(_abi.hcRefineSettings()) == before and call(other) == before
