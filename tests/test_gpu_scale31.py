"""GPU tests of the scale fit (include/scale/hc_pose_scale.h), a mode of the
four refine calls.  The rule is integer-exact float32, so everything is compared
exactly with the numpy reference (tests/scale_reference.py): the scale's bits,
the voter, the counts, the key and the transfer mask's words.

Scenes: "clean", the noiseless edgels of dataset 000 under the GT pose turned by
3e-4 rad, cut to the sizes around the wave width and voter tile (64), the vote's
workgroup (512 threads) and the LDS stage (2048 edgels); "noisy", the config-5
fixture (the joint winner of pose_joint_noisy1px_N100.npz on the 5117 edgels
with 1 px noise); and the eight refined candidates of trial 12
(pose_topk_noisy1px_trial12_N100.npz).
"""
import ctypes as C

import numpy as np
import pytest

import graph_common as G
import refine_reference as RR
import scale_reference as SR
from checks import NOISE_SEED, golden, noisy_data
from refine_reference import POSE_KEYS, gt_pose, perturbed

pytestmark = pytest.mark.gpu

# the wave width = the voter tile (64), several tiles (257), the staging stride of the vote's 512 threads, the LDS
# stage (2048 edgels), several stages and every wave's slice of a stage (5117)
SIZES = [1, 2, 63, 64, 65, 257, 511, 512, 513, 2048, 2049, 5117]
TRUE_SCALE = 1.1852790          # dataset 000, tests/test_scale31_host.py
REPORT_KEYS = ("status", "num_voters", "voter", "transfer_inliers", "tested", "joint", "key")


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


SCALE_OFFSET = 128      # hcTrifocalSelection::scale31


def _same_apart_from_scale(a: bytes, b: bytes):
    return a[:SCALE_OFFSET] == b[:SCALE_OFFSET] and a[SCALE_OFFSET + 4:] == b[SCALE_OFFSET + 4:]


def _assert_report(rep, ref, what=""):
    """A device scale report (dict) against the reference's, exactly."""
    for k in REPORT_KEYS:
        assert rep[k] == ref[k], (what, k, rep[k], ref[k])
    assert np.float32(rep["scale31"]).tobytes() == np.float32(ref["scale31"]).tobytes(), (what, rep["scale31"], ref["scale31"])
    assert np.float32(rep["scale_in"]).tobytes() == np.float32(ref["scale_in"]).tobytes(), what
    if "mask" in rep:
        assert np.array_equal(rep["mask"], SR.pack(ref["mask"])), what
        assert _popcount(rep["mask"]) == rep["transfer_inliers"], what


@pytest.fixture(scope="module")
def scenes(tracker, ransac0):
    """Per scene kind: the host edgels, their device copy, K and the input pose."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = tracker.device
    noisy0 = noisy_data()
    g = golden("pose_joint_noisy1px_N100")
    i = int(np.nonzero(g["cand_ids"] == g["path"])[0][0])
    # the winner's pose as the device converts it: the joint call over its track alone
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
                          pose=perturbed(gt_pose(ransac0)), data=ransac0),
            "gt": dict(loc=ransac0.locations, dev=_dev(np.array(ransac0.locations), dev), K=ransac0.K, Kdev=K,
                       pose=gt_pose(ransac0), data=ransac0)}


def _case(scenes, kind, E, **kw):
    s = scenes[kind]
    return _selection(s["pose"], s["loc"][:E], s["K"], **kw), s["dev"][:E], s["Kdev"], s["loc"][:E]


# ---- the scale-only call on small scenes ------------------------------------------------------------

@pytest.mark.parametrize("E", SIZES)
def test_small_scenes_equal_the_reference(scenes, E):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, K, loc = _case(scenes, "clean", E)
    ref = SR.fit(sel, loc, scenes["clean"]["K"], scale_in=sel["scale31"])
    in_dev = _upload(sel, edgels.device)
    keep = _bytes(in_dev)
    out_dev, rep_dev, words = pose.launch_fit_scale31(in_dev, edgels, K, transfer_mask=True)
    out, rep = pose.fit_scale31(in_dev, edgels, K, transfer_mask=True)
    print(f"clean E={E}: scale {rep['scale31']!r} | {ref['scale31']!r}, voter {rep['voter']} | {ref['voter']}, "
          f"transfer {rep['transfer_inliers']} | {ref['transfer_inliers']} of {rep['tested']} | {ref['tested']}")
    assert ref["status"] == 0 and ref["joint"] == E                 # under a pixel off: every edgel is a joint inlier
    assert abs(float(ref["scale31"]) - TRUE_SCALE) < 0.01
    _assert_report(rep, ref, E)
    assert _bytes(in_dev) == keep and _same_apart_from_scale(_bytes(out_dev), keep)
    assert out["scale31"].tobytes() == np.float32(ref["scale31"]).tobytes()
    assert _struct_bytes(out) == _bytes(out_dev)
    assert pose.scale_report_dict(rep_dev) == {k: v for k, v in rep.items() if k != "mask"}
    assert len(rep["mask"]) == (E + 63) // 64 and np.array_equal(words.cpu().numpy().view(np.uint64), rep["mask"])
    # out == in is allowed
    alias = in_dev.clone()
    o2, r2, _ = pose.launch_fit_scale31(alias, edgels, K, out=alias)
    assert o2.data_ptr() == alias.data_ptr() and _bytes(alias) == _bytes(out_dev) and _bytes(r2) == _bytes(rep_dev)


def _behind_camera_scene(data):
    """One edgel that both two-view tests accept and whose depth in view 1 is
    negative: the first clean edgel's point mirrored through the first camera's
    centre, projected into views 2 and 3 under the GT pose at the true scale."""
    gt = gt_pose(data)
    P = SR._pose(gt, np.float64)
    rho, _, _, _ = SR._edgels(data.locations[:1], data.K, P, np.float64)
    g = data.locations[0, 0:2].astype(np.float64)
    X = -rho[0] * np.array([g[0], g[1], 1.0])
    x2 = P[0].reshape(3, 3) @ X + P[1]
    x3 = P[2].reshape(3, 3) @ X + TRUE_SCALE * P[3]
    loc = np.array([[g[0], g[1], x2[0] / x2[2], x2[1] / x2[2], x3[0] / x3[2], x3[1] / x3[2]]], np.float32)
    return gt, loc


def test_no_voter_and_no_path_leave_the_scale_as_copied(scenes, ransac0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    dev = scenes["clean"]["dev"].device
    Kd, K = scenes["clean"]["Kdev"], ransac0.K
    # no joint inlier: view 3 far off
    far = np.array(ransac0.locations[:65])
    far[:, 4:6] += 0.5
    # one joint inlier with rho <= 0, constructed with the reference
    gt, behind = _behind_camera_scene(ransac0)
    for name, pose32, loc, joint in (("far", scenes["clean"]["pose"], far, 0), ("behind", gt, behind, 1)):
        sel = _selection(pose32, loc, K, scale31=3.5)
        ref = SR.fit(sel, loc, K, scale_in=3.5)
        assert (ref["status"], ref["joint"], ref["tested"], ref["num_voters"]) == (SR.NO_VOTER, joint, 0, 0), name
        assert sel["inliers"] == joint
        in_dev = _upload(sel, dev)
        out_dev, rep_dev, words = pose.launch_fit_scale31(in_dev, _dev(loc, dev), Kd, transfer_mask=True)
        rep = pose.scale_report_dict(rep_dev)
        assert rep["status"] == _abi.HC_SCALE_NO_VOTER and rep["no_voter"] and not rep["none"], name
        _assert_report(rep, ref, name)
        assert _bytes(out_dev) == _bytes(in_dev) and float(rep["scale31"]) == 3.5, name
        assert not words.cpu().numpy().any(), name
    # no path
    none = pose.joint_selection_dict(_abi.hcTrifocalSelection())
    none.update(path=-1, inliers=-1, inliers21=-1, inliers31=-1, scale31=np.float32(0.0))
    in_dev = _upload(none, dev)
    out_dev, rep_dev, words = pose.launch_fit_scale31(in_dev, scenes["clean"]["dev"][:257], Kd, transfer_mask=True)
    rep = pose.scale_report_dict(rep_dev)
    _assert_report(rep, SR.fit(scenes["clean"]["pose"], ransac0.locations[:257], K, has_path=False), "none")
    assert rep["status"] == _abi.HC_SCALE_NONE and _bytes(out_dev) == _bytes(in_dev) and not words.cpu().numpy().any()
    # with the refinement in the same call: both reports say none
    out, r = pose.refine_joint(in_dev, scenes["clean"]["dev"][:257], Kd, fit_scale=True)
    assert r["none"] and r["scale"]["none"] and out["path"] == -1


def test_ties_go_to_the_last_voter(scenes):
    """The clean 257 edgels under the exact GT pose: every voter's scale puts
    all 257 within 2 px, so the key decides: the last voter."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, K, loc = _case(scenes, "gt", 257)
    ref = SR.fit(sel, loc, scenes["gt"]["K"], scale_in=sel["scale31"])
    assert ref["num_voters"] == 257 and (ref["counts"] == 257).all()
    _, rep = pose.fit_scale31(sel, edgels, K, transfer_mask=True)
    _assert_report(rep, ref, "ties")
    assert rep["voter"] == 256 and rep["key"] == (257 << 32) | 256


# ---- the config-5 fixture -------------------------------------------------------------------------

def test_noisy_fixture_scale_only(scenes):
    """The joint winner of the fixture: the CPU float64 prediction is 1.228 with
    614 of 1133; the float32 reference decides the exact integers."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    s = scenes["noisy"]
    sel, edgels, K = s["pose"], s["dev"], s["Kdev"]
    ref = SR.fit(sel, s["loc"], s["K"], scale_in=sel["scale31"])
    in_dev = _upload(sel, edgels.device)
    out_dev, rep_dev, words = pose.launch_fit_scale31(in_dev, edgels, K, transfer_mask=True)
    rep = pose.scale_report_dict(rep_dev)
    rep["mask"] = words.cpu().numpy().view(np.uint64)
    print(f"noisy fixture: solver ratio {sel['scale31']!r}, fitted {rep['scale31']!r} | {ref['scale31']!r}, "
          f"transfer {rep['transfer_inliers']} | {ref['transfer_inliers']} of {rep['joint']} joint, voter {rep['voter']}")
    assert abs(float(sel["scale31"]) - 22.82) < 0.01
    assert (ref["joint"], ref["transfer_inliers"]) == (1133, 614) and abs(float(ref["scale31"]) - 1.228) < 5e-4
    _assert_report(rep, ref, "noisy")
    assert _same_apart_from_scale(_bytes(out_dev), _bytes(in_dev))
    assert _bytes(out_dev)[SCALE_OFFSET:SCALE_OFFSET + 4] == np.float32(ref["scale31"]).tobytes()
    joint = pose.inlier_mask(out_dev, edgels, K, packed=True)
    assert _popcount(rep["mask"]) == rep["transfer_inliers"] and not (rep["mask"] & ~joint).any()
    assert _popcount(joint) == rep["joint"] == 1133


def test_noisy_fixture_refined_and_fitted_in_one_call(scenes):
    """Ten Gauss-Newton iterations and the fit in one call: out is the plain
    call's with only scale31 replaced, and the fit is the reference's on the
    pose that came out."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    s = scenes["noisy"]
    sel, edgels, K = s["pose"], s["dev"], s["Kdev"]
    in_dev = _upload(sel, edgels.device)
    plain, plain_rep = pose.launch_refine_joint(in_dev, edgels, K, iterations=10)
    out_dev, report, scale, words = pose.launch_refine_joint(in_dev, edgels, K, iterations=10, fit_scale=True,
                                                             transfer_mask=True)
    out, rep = pose.refine_joint(in_dev, edgels, K, iterations=10, fit_scale=True, transfer_mask=True)
    assert _bytes(report) == _bytes(plain_rep) and _same_apart_from_scale(_bytes(out_dev), _bytes(plain))
    assert _struct_bytes(out) == _bytes(out_dev)
    assert {k: v for k, v in rep["scale"].items() if k != "mask"} == pose.scale_report_dict(scale)
    ref = SR.fit(out, s["loc"], s["K"], scale_in=sel["scale31"])
    print(f"noisy fixture refined: {out['inliers']} joint, fitted {rep['scale']['scale31']!r} | {ref['scale31']!r}, "
          f"transfer {rep['scale']['transfer_inliers']} | {ref['transfer_inliers']}")
    _assert_report(rep["scale"], ref, "refined")
    assert rep["scale"]["joint"] == out["inliers"] > 3000
    assert out["scale31"].tobytes() == np.float32(ref["scale31"]).tobytes()
    joint = pose.inlier_mask(out_dev, edgels, K, packed=True)
    assert not (rep["scale"]["mask"] & ~joint).any()
    assert np.array_equal(words.cpu().numpy().view(np.uint64), rep["scale"]["mask"])
    assert abs(float(out["scale31"]) - TRUE_SCALE) < 0.02


def test_mode_off_is_the_call_as_it_was(scenes):
    """Zeroed settings, the Python defaults and a pad the mode does not know give
    the same bytes, before and after a scale-mode call on the same buffers."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    sel, edgels, K, _ = _case(scenes, "noisy", 2049)
    dev = edgels.device
    in_dev = _upload(sel, dev)
    out = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    report = torch.empty(pose.REPORT_BYTES, dtype=torch.uint8, device=dev)

    def call(settings):
        G.poison(out, report)
        _abi.call("hc_trifocal_pose_refine", _abi.ptr(in_dev), 2049, _abi.ptr(edgels), _abi.ptr(K),
                  C.byref(settings) if settings is not None else None, _abi.ptr(out), _abi.ptr(report),
                  _abi.ptr(torch.cuda.current_stream(dev)))
        torch.cuda.synchronize(dev)
        return _bytes(out), _bytes(report)
    other = _abi.hcRefineSettings()
    other.pad[0], other.pad[1] = 0x12345, 3
    before = call(_abi.hcRefineSettings())
    assert call(None) == before and call(other) == before
    o, r = pose.launch_refine_joint(in_dev, edgels, K)
    assert (_bytes(o), _bytes(r)) == before
    # a scale-mode call into the same buffers
    ss = _abi.hcRefineScaleSettings()
    ss.head.pad[0] = _abi.HC_REFINE_SCALE31
    scale = torch.empty(pose.SCALE_REPORT_BYTES, dtype=torch.uint8, device=dev)
    ss.reports = scale.data_ptr()
    _abi.call("hc_trifocal_pose_refine", _abi.ptr(in_dev), 2049, _abi.ptr(edgels), _abi.ptr(K),
              C.cast(C.pointer(ss), C.POINTER(_abi.hcRefineSettings)), _abi.ptr(out), _abi.ptr(report),
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    assert _same_apart_from_scale(_bytes(out), before[0]) and _bytes(out) != before[0] and _bytes(report) == before[1]
    assert pose.scale_report_dict(scale)["status"] == 0
    assert call(_abi.hcRefineSettings()) == before and call(other) == before


# ---- trial 12: the eight refined candidates ---------------------------------------------------------

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
    return dict(g=g, data=data, edgels=edgels, K=K, tracks=T, conv=Cv, cand=cand)


def test_trial12_topk_fit_and_selection(trial12):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    c = trial12
    S = pose.JOINT_SEL_BYTES
    plain = pose.launch_refine_topk(c["cand"], c["edgels"], c["K"])
    best, rank, refined, reports, scale = pose.launch_refine_topk(c["cand"], c["edgels"], c["K"], fit_scale=True)
    # the refinement and today's selection are untouched: only scale31 differs
    assert _bytes(rank) == _bytes(plain[1]) and _bytes(reports) == _bytes(plain[3])
    rf, pf = _bytes(refined), _bytes(plain[2])
    for r in range(8):
        assert _same_apart_from_scale(rf[r * S:(r + 1) * S], pf[r * S:(r + 1) * S]), r
    rk = int(rank.cpu().numpy()[0])
    assert _same_apart_from_scale(_bytes(best), _bytes(plain[0])) and _bytes(best) == rf[rk * S:(rk + 1) * S]
    bd, br, rd, pd = pose.refine_topk(c["cand"], c["edgels"], c["K"], fit_scale=True)
    assert br == rk and rk in (2, 4, 6)
    # all eight fits are the reference's on the device's refined poses
    keys = []
    ratios = [pose.joint_selection_dict(pose.joint_selection_struct(row))["scale31"]
              for row in c["cand"].cpu().numpy().reshape(8, S)]            # the solver's ratios, as they came in
    for r, (d, p) in enumerate(zip(rd, pd)):
        ref = SR.fit(d, c["data"].locations, c["data"].K, scale_in=ratios[r])
        print(f"trial 12 rank {r} path {d['path']}: joint {d['inliers']}, fitted {p['scale']['scale31']!r} | "
              f"{ref['scale31']!r}, transfer {p['scale']['transfer_inliers']} | {ref['transfer_inliers']}")
        _assert_report(p["scale"], ref, r)
        assert d["scale31"].tobytes() == np.float32(ref["scale31"]).tobytes() and p["scale"]["joint"] == d["inliers"]
        keys.append((ref["transfer_inliers"] << 32) | d["path"])
    # the right basin (ranks 2, 4, 6) is separated more sharply than by the joint count
    right = [keys[r] >> 32 for r in (2, 4, 6)]
    wrong = [keys[r] >> 32 for r in (0, 1, 3, 5, 7)]
    assert min(right) > 2000 and max(wrong) < 1000
    for r in (2, 4, 6):
        assert abs(float(rd[r]["scale31"]) - TRUE_SCALE) < 0.02
    # by transfer: the entry with the largest transfer key, and it passes the GT check
    bt, rt, rdt, pdt = pose.refine_topk(c["cand"], c["edgels"], c["K"], fit_scale=True, select_by_transfer=True,
                                        transfer_mask=True)
    assert rt == int(np.argmax(keys)) and rt in (2, 4, 6)
    assert _struct_bytes(bt) == _struct_bytes(rdt[rt]) == _struct_bytes(rd[rt])
    res, ok = pose.residuals(c["data"], bt)
    assert ok and res[0] < 0.1 and res[1] < 0.1
    assert _popcount(pdt[rt]["scale"]["mask"]) == pdt[rt]["scale"]["transfer_inliers"] == keys[rt] >> 32
    # the whole chain on one stream
    b2, info = pose.select_refined(c["tracks"], c["conv"], c["edgels"], c["K"], k=8, fit_scale=True,
                                   select_by_transfer=True)
    assert _struct_bytes(b2) == _struct_bytes(bt) and info["best_rank"] == rt
    assert info["scale"] == {k: v for k, v in pdt[rt]["scale"].items() if k != "mask"}


# ---- grouped ----------------------------------------------------------------------------------------

def test_grouped_equals_single_calls(problem, scenes):
    """Two triplets of different E, 65 and 2049, in one launch: every report is
    the single call's on that triplet alone; the same through the grouped top-k
    call with two candidates per triplet."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    kinds = [("clean", 65), ("noisy", 2049)]
    batch = TripletBatch(problem, [scenes[k]["data"] for k, _ in kinds], seeds=0, samples_per_triplet=1,
                         edgel_counts=[E for _, E in kinds])
    cases = [_case(scenes, k, E, path=100 + i, num_candidates=3 + i) for i, (k, E) in enumerate(kinds)]
    dev = cases[0][1].device
    db = batch.to(dev)
    sels, reps, scales = pose.launch_refine_joint_grouped([c[0] for c in cases], db, fit_scale=True)
    torch.cuda.synchronize(dev)
    S, R, Q = pose.JOINT_SEL_BYTES, pose.REPORT_BYTES, pose.SCALE_REPORT_BYTES
    singles = []
    for t, (sel, edgels, K, loc) in enumerate(cases):
        one, rep, scale, _ = pose.launch_refine_joint(sel, edgels, K, fit_scale=True)
        assert _bytes(sels)[t * S:(t + 1) * S] == _bytes(one), t
        assert _bytes(reps)[t * R:(t + 1) * R] == _bytes(rep), t
        assert _bytes(scales)[t * Q:(t + 1) * Q] == _bytes(scale), t
        d = pose.joint_selection_dict(pose.joint_selection_struct(one))
        _assert_report(pose.scale_report_dict(scale), SR.fit(d, loc, scenes["clean"]["K"], scale_in=sel["scale31"]), t)
        singles.append((one, scale))
    dicts, reports = pose.refine_joint_grouped([c[0] for c in cases], batch, device=dev, fit_scale=True)
    assert [r["scale"] for r in reports] == [pose.scale_report_dict(s) for _, s in singles]
    # top-k, grouped: per triplet the selection itself and a second candidate that is "none"
    none = dict(cases[0][0], path=-1)
    cand = [cases[0][0], none, cases[1][0], dict(cases[1][0], path=7)]
    out = pose.refine_topk_grouped(cand, db, 2, fit_scale=True, select_by_transfer=True)
    for t in range(2):
        assert out[t]["reports"][0]["scale"] == pose.scale_report_dict(singles[t][1]), t
        assert _struct_bytes(out[t]["refined"][0]) == _bytes(singles[t][0]), t
    assert out[0]["reports"][1]["scale"]["none"] and out[0]["best_rank"] == 0
    # equal transfer counts: the larger path wins (the key is transfer_inliers << 32 | path)
    assert out[1]["reports"][1]["scale"]["transfer_inliers"] == out[1]["reports"][0]["scale"]["transfer_inliers"]
    assert out[1]["best_rank"] == 0 and out[1]["best"]["path"] == 101
    with pytest.raises(Exception):
        pose.launch_refine_topk_grouped(cand, db, 2, fit_scale=True, transfer_mask=True)


# ---- graph capture and replay -------------------------------------------------------------------------

def test_graph_replay_of_the_fit(scenes):
    """launch_refine_joint(fit_scale=True) recorded once and replayed twice:
    both replays give the eager call's bytes, with every output poisoned from
    outside the graph before each replay -- the vote's key word included: the
    call's own kernels reset it."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, K, _ = _case(scenes, "noisy", 2049)
    in_dev = _upload(sel, edgels.device)

    def enqueue():
        return pose.launch_refine_joint(in_dev, edgels, K, fit_scale=True, transfer_mask=True)
    eager = [_bytes(t) for t in enqueue()]
    cap, out = G.capture(enqueue)
    try:
        for _ in range(2):
            G.poison(*out)
            cap.replay()
            torch.cuda.synchronize()
            assert [_bytes(t) for t in out] == eager
            assert pose.scale_report_dict(out[2])["status"] == 0
    finally:
        G.release(cap)
