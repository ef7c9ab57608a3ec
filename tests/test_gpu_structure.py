"""GPU tests of the structure stage (include/structure/hc_pose_structure.h), the
fourth stage of the four refine calls.  Every float of the rule is defined to
the bit, so the device's records and reports are compared with the numpy
reference (tests/structure_reference.py) byte for byte; in the full mode the
reference is applied to the device's own output pose, so a difference is the
stage's alone.

Scenes: "clean", the noiseless edgels of dataset 000 under the GT pose with the
voted scale, cut to the sizes either side of the wave (64) and of the tile of
256 edgels the ranking walks, and whole (5117: twenty tiles); "noisy", the
config-5 fixture (the joint winner of pose_joint_noisy1px_N100.npz on the 5117
edgels with 1 px noise; structure-only after its two-view refinement and scale
vote), where W is a strict subset; the eight candidates of
trial 12 (pose_topk_noisy1px_trial12_N100.npz).
"""
import numpy as np
import pytest

import graph_common as G
import refine_reference as RR
import scale_reference as SR
import structure_reference as ST
from checks import NOISE_SEED, golden, noisy_data
from refine_reference import POSE_KEYS, gt_pose

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 5117]
REPORT_KEYS = ("status", "count", "tangents", "oriented")


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


def _sentinel(entries, dev):
    """A records buffer of that many hcEdgel3D filled with the poison byte."""
    import torch
    return torch.full((entries * 48,), G.POISON_BYTE, dtype=torch.uint8, device=dev)


def _same_report(rep, ref, what):
    assert {k: rep[k] for k in REPORT_KEYS} == {k: ref[k] for k in REPORT_KEYS}, what
    assert np.float32(rep["scale31"]).tobytes() == np.float32(ref["scale31"]).tobytes(), what


def _against_reference(what, rec, rep, sel, loc, tan, K, **kw):
    """Device records (a structured array) and report dict against the float32
    reference under the selection's floats: every field of every record."""
    ref, rrep = ST.reconstruct(sel, sel["scale31"], loc, tan, K, **kw)
    t = (ref["flags"] & ST.TANGENT) != 0
    print(f"{what}: count {rep['count']} | {rrep['count']} of {len(loc)}, tangents {rep['tangents']} | "
          f"{rrep['tangents']}, oriented {rep['oriented']} | {rrep['oriented']}, median sin3 "
          f"{float(np.median(ref['sin3'][t])) if t.any() else float('nan'):.3e}")
    _same_report(rep, rrep, what)
    assert rec.dtype == ref.dtype and len(rec) == len(ref), what
    for k in ref.dtype.names if len(ref) else ():
        bad = np.nonzero((rec[k].reshape(len(rec), -1).view(np.uint32) !=
                          ref[k].reshape(len(ref), -1).view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} records, first {bad[:5].tolist()}: " \
                              f"{rec[k][bad[:2]].tolist()} | {ref[k][bad[:2]].tolist()}"
    assert rec.tobytes() == ref.tobytes(), what
    return ref, rrep


@pytest.fixture(scope="module")
def scenes(tracker, ransac0):
    """Per scene kind: the host edgels and tangents, their device copies, K and the pose."""
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
    assert np.array_equal(noisy0.tangents, ransac0.tangents)
    # the winner carries the minimal solver's scale31, under which no edgel transfers; the structure-only cases
    # take stages 1 and 2 of it, the two-view refinement with the voted scale
    two_dev, *_ = pose.launch_refine_joint(_upload(winner, dev), noisy_dev, K, fit_scale=True)
    fitted = pose.joint_selection_dict(pose.joint_selection_struct(two_dev))
    gt = gt_pose(ransac0)
    gt["scale31"] = SR.fit(gt, ransac0.locations, ransac0.K)["scale31"]
    tan_dev = _dev(np.array(ransac0.tangents), dev)
    return {"noisy": dict(loc=noisy0.locations, tan=noisy0.tangents, dev=noisy_dev, tan_dev=tan_dev, K=noisy0.K,
                          Kdev=K, pose=fitted, winner=winner, data=noisy0),
            "clean": dict(loc=ransac0.locations, tan=ransac0.tangents, dev=_dev(np.array(ransac0.locations), dev),
                          tan_dev=tan_dev, K=ransac0.K, Kdev=K, pose=gt, data=ransac0)}


def _case(scenes, kind, E, **kw):
    s = scenes[kind]
    kw.setdefault("scale31", s["pose"]["scale31"])
    sel = _selection(s["pose"], s["loc"][:E], s["K"], **kw)
    return sel, s["dev"][:E], s["tan_dev"][:E], s["Kdev"], s["loc"][:E], s["tan"][:E]


# ---- the structure-only mode against the reference ---------------------------------------------------

@pytest.mark.parametrize("kind,E", [("clean", E) for E in SIZES] + [("noisy", 5117), ("noisy", 300)])
def test_reconstruct_against_the_reference(scenes, kind, E):
    """HC_STRUCTURE_ONLY: out is in, every record and the report are the
    reference's bits, and nothing is written at or beyond count."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, tangents, K, loc, tan = _case(scenes, kind, E)
    dev = edgels.device
    in_dev = _upload(sel, dev)
    keep = _bytes(in_dev)
    buf = _sentinel(E + 3, dev)
    out, rec_dev, srep = pose.launch_reconstruct(in_dev, edgels, tangents, K, edgels3d=buf)
    rep = pose.structure_report_dict(srep)
    rec = pose.structure_records(rec_dev, rep)
    assert rec_dev.data_ptr() == buf.data_ptr() and _bytes(out) == keep == _bytes(in_dev)
    ref, rrep = _against_reference(f"{kind} E={E}", rec, rep, sel, loc, tan, scenes[kind]["K"])
    assert G.is_poisoned(buf[rep["count"] * 48:])
    assert np.array_equal(rec["edgel"], np.nonzero(ST.transfer_set(sel, sel["scale31"], loc, scenes[kind]["K"]))[0])
    if kind == "clean":
        assert rep["count"] == E and (rec["err3_px"] < 0.01).all()
        t = (rec["flags"] & 1) != 0
        assert (rec["sin3"][t] < 1e-4).all() and rep["oriented"] == rep["tangents"] == int(t.sum())
    else:
        assert 0 < rep["count"] < E and rep["oriented"] <= rep["tangents"] <= rep["count"]
    # the synchronous form, thresholds of its own, and out == in
    rec2, rep2 = pose.reconstruct(in_dev, edgels, tangents, K, min_sin_plane=0.25, max_sin3=1e-6)
    _against_reference(f"{kind} E={E}, thresholds", rec2, rep2, sel, loc, tan, scenes[kind]["K"], min_sin_plane=0.25,
                       max_sin3=1e-6)
    assert rep2["count"] == rep["count"] and rep2["tangents"] <= rep["tangents"]
    alias = in_dev.clone()
    o2, r2, s2 = pose.launch_reconstruct(alias, edgels, tangents, K, out=alias)
    assert o2.data_ptr() == alias.data_ptr() and _bytes(alias) == keep
    assert _bytes(s2) == _bytes(srep) and _bytes(r2)[:rep["count"] * 48] == rec.tobytes()


# ---- the full mode on the fixture -------------------------------------------------------------------

def test_full_mode_on_the_fixture(scenes):
    """The three stages are the three_view call's, byte for byte; the records
    are the reference's under the device's own output pose, and their edgels
    are the transfer mask's bits."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    s = scenes["noisy"]
    edgels, tangents, K = s["dev"], s["tan_dev"], s["Kdev"]
    in_dev = _upload(s["winner"], edgels.device)
    three = pose.launch_refine_joint(in_dev, edgels, K, three_view=True, transfer_mask=True)
    buf = _sentinel(5117, edgels.device)
    full = pose.launch_refine_joint(in_dev, edgels, K, structure=True, tangents=tangents, transfer_mask=True,
                                    edgels3d=buf)
    assert [_bytes(t) for t in full[:5]] == [_bytes(t) for t in three]
    out = pose.joint_selection_dict(pose.joint_selection_struct(full[0]))
    rep = pose.structure_report_dict(full[6])
    rec = pose.structure_records(full[5], rep)
    tv = pose.three_view_report_dict(full[4])
    _against_reference("noisy fixture, full mode", rec, rep, out, s["loc"], s["tan"], s["K"])
    mask = np.unpackbits(full[3].cpu().numpy().view(np.uint8), bitorder="little")[:5117].astype(bool)
    assert np.array_equal(rec["edgel"], np.nonzero(mask)[0]) and rep["count"] == tv["transfer_inliers"] >= 2700
    assert tv["best_iteration"] > 0 and G.is_poisoned(buf[rep["count"] * 48:])
    t = (rec["flags"] & 1) != 0
    print(f"    median sin3 {np.median(rec['sin3'][t]):.3e}, oriented {rep['oriented']} of {rep['tangents']}")
    assert np.median(rec["sin3"][t]) < 1e-3 and rep["oriented"] > 0.95 * rep["tangents"]
    # the synchronous wrapper returns the same, the structure beside the report
    o2, r2, st2 = pose.refine_joint(in_dev, edgels, K, structure=True, tangents=tangents)
    assert _struct_bytes(o2) == _bytes(full[0]) and r2["structure"] == rep and st2.tobytes() == rec.tobytes()
    assert r2["three_view"]["transfer_history"].tolist() == tv["transfer_history"].tolist()
    # and equals the structure-only call on the selection that went out
    rec3, rep3 = pose.reconstruct(full[0], edgels, tangents, K)
    assert rec3.tobytes() == rec.tobytes() and rep3 == rep


# ---- trial 12: the eight candidates through the top-k call -----------------------------------------

@pytest.fixture(scope="module")
def trial12(tracker, ransac0):
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
    return dict(data=data, edgels=edgels, K=K, tracks=T, conv=Cv, cand=cand,
                tangents=_dev(np.array(data.tangents), dev))


@pytest.mark.parametrize("by_transfer", [False, True])
def test_trial12_topk_structure_is_that_of_best(trial12, by_transfer):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    c = trial12
    kw = dict(select_by_transfer=True) if by_transfer else {}
    three = pose.launch_refine_topk(c["cand"], c["edgels"], c["K"], three_view=True, **kw)
    full = pose.launch_refine_topk(c["cand"], c["edgels"], c["K"], structure=True, tangents=c["tangents"], **kw)
    assert [_bytes(t) for t in full[:6]] == [_bytes(t) for t in three]
    best, rank, refined, reports, srep, rec = pose.refine_topk(c["cand"], c["edgels"], c["K"], structure=True,
                                                               tangents=c["tangents"], **kw)
    assert rank in (2, 4, 6) and _struct_bytes(best) == _bytes(full[0])
    assert srep == pose.structure_report_dict(full[7]) and rec.tobytes() == pose.structure_records(full[6], srep).tobytes()
    assert srep["status"] == 0 and srep["count"] == reports[rank]["three_view"]["transfer_inliers"] >= 2690
    rec1, rep1 = pose.reconstruct(best, c["edgels"], c["tangents"], c["K"])
    assert rec1.tobytes() == rec.tobytes() and rep1 == srep
    _against_reference(f"trial 12, best rank {rank}", rec, srep, best, c["data"].locations, c["data"].tangents,
                       c["data"].K)
    # the whole chain on one stream
    b2, info = pose.select_refined(c["tracks"], c["conv"], c["edgels"], c["K"], k=8, structure=True,
                                   tangents=c["tangents"], **kw)
    assert _struct_bytes(b2) == _struct_bytes(best) and info["best_rank"] == rank
    assert info["structure_report"] == srep and info["structure"].tobytes() == rec.tobytes()


# ---- grouped ----------------------------------------------------------------------------------------

def test_grouped_equals_single_calls(problem, scenes):
    """Four triplets of 65, 2049, 17 and 129 edgels in one launch: every
    triplet's selection, reports and records, at its edgel_offsets slot, are the
    single call's on that triplet alone, bit for bit, in the full mode, in the
    structure-only mode and through the grouped top-k call; the entries between
    a triplet's count and the next triplet's slot keep the caller's bytes."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    kinds = [("clean", 65), ("noisy", 2049), ("clean", 17), ("clean", 129)]
    batch = TripletBatch(problem, [scenes[k]["data"] for k, _ in kinds], seeds=0, samples_per_triplet=1,
                         edgel_counts=[E for _, E in kinds])
    cases = [_case(scenes, k, E, path=100 + i, num_candidates=3 + i) for i, (k, E) in enumerate(kinds)]
    dev = cases[0][1].device
    db = batch.to(dev)
    offs = [0, 65, 65 + 2049, 65 + 2049 + 17]
    total = offs[-1] + 129
    assert db.edgel_offsets_device.cpu().numpy().tolist() == offs == db.edgel_offsets.tolist()
    assert db.edgel_offsets_device.dtype == torch.int32 and tuple(db.tangents.shape) == (total, 6)
    assert np.array_equal(db.tangents.cpu().numpy(), np.concatenate([c[5] for c in cases]))
    sels = [c[0] for c in cases]
    for only in (False, True):
        buf = _sentinel(total, dev)
        if only:
            g_out, g_rec, g_srep = pose.launch_reconstruct_grouped(sels, db, edgels3d=buf)
            g_rest = []
        else:
            g_out, *g_rest, g_rec, g_srep = pose.launch_refine_joint_grouped(sels, db, structure=True,
                                                                             three_view_iterations=6, edgels3d=buf)
        torch.cuda.synchronize(dev)
        raw, S, B = _bytes(g_rec), pose.JOINT_SEL_BYTES, pose.STRUCTURE_REPORT_BYTES
        for t, (sel, edgels, tangents, K, loc, tan) in enumerate(cases):
            if only:
                one, rec, srep = pose.launch_reconstruct(sel, edgels, tangents, K)
                assert _bytes(one) == _struct_bytes(sel), t
                rest = []
            else:
                one, *rest, rec, srep = pose.launch_refine_joint(sel, edgels, K, structure=True, tangents=tangents,
                                                                 three_view_iterations=6)
            assert _bytes(g_out)[t * S:(t + 1) * S] == _bytes(one), (only, t)
            assert _bytes(g_srep)[t * B:(t + 1) * B] == _bytes(srep), (only, t)
            for a, b in zip(g_rest, [r for r in rest if r is not None]):
                n = b.numel()
                assert _bytes(a)[t * n:(t + 1) * n] == _bytes(b), (only, t)
            rep = pose.structure_report_dict(srep)
            n = rep["count"]
            assert 0 < n <= kinds[t][1] and raw[offs[t] * 48:(offs[t] + n) * 48] == _bytes(rec)[:n * 48], (only, t)
            assert G.is_poisoned(buf[(offs[t] + n) * 48:(offs[t] + kinds[t][1]) * 48]), (only, t)
            out = pose.joint_selection_dict(pose.joint_selection_struct(one))
            _against_reference(f"grouped t={t} only={only}", pose.structure_records(rec, rep), rep, out, loc, tan,
                               scenes[kinds[t][0]]["K"])
    # the synchronous wrappers
    dicts, reports, structs = pose.refine_joint_grouped(sels, batch, device=dev, structure=True,
                                                        three_view_iterations=6)
    recs, reps = pose.reconstruct_grouped(dicts, db)
    for t in range(4):
        assert reports[t]["structure"] == reps[t] and structs[t].tobytes() == recs[t].tobytes(), t
        assert len(structs[t]) == reps[t]["count"] > 0, t
    # top-k, grouped: per triplet the selection itself and a second candidate ("none", or the same pose at another path)
    none = dict(sels[0], path=-1)
    cand = [sels[0], none, sels[1], dict(sels[1], path=7), sels[2], sels[2], sels[3], none]
    for kw in (dict(), dict(select_by_transfer=True)):
        out = pose.refine_topk_grouped(cand, db, 2, structure=True, three_view_iterations=6, **kw)
        for t in range(4):
            assert _struct_bytes(out[t]["best"]) == _struct_bytes(dicts[t]), t
            assert out[t]["structure_report"] == reps[t] and out[t]["structure"].tobytes() == recs[t].tobytes(), t
    # every candidate of triplet 0 without a path: no best, nothing to reconstruct there
    out = pose.refine_topk_grouped([none, none] + cand[2:], db, 2, structure=True, three_view_iterations=6)
    assert out[0]["best_rank"] == -1 and out[0]["structure_report"]["none"] and len(out[0]["structure"]) == 0
    assert out[1]["structure"].tobytes() == recs[1].tobytes()


# ---- nothing to reconstruct ------------------------------------------------------------------------

def test_no_path_and_no_voter_give_none(scenes, ransac0):
    """Without a path, and on the scale tests' scene without a voter (view 3
    moved far off) in the full mode: HC_STRUCTURE_NONE, count 0, no record
    written."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    dev = scenes["clean"]["dev"].device
    Kd, K = scenes["clean"]["Kdev"], ransac0.K
    none = pose.joint_selection_dict(_abi.hcTrifocalSelection())
    none.update(path=-1, inliers=-1, inliers21=-1, inliers31=-1, scale31=np.float32(0.5))
    far = np.array(ransac0.locations[:65])
    far[:, 4:6] += 0.5
    sel = _selection(scenes["clean"]["pose"], far, K, scale31=3.5)
    assert SR.fit(sel, far, K, scale_in=3.5)["status"] == SR.NO_VOTER
    tangents = scenes["clean"]["tan_dev"]
    for name, s, edgels, E in (("none", none, scenes["clean"]["dev"][:257], 257), ("far", sel, _dev(far, dev), 65)):
        in_dev = _upload(s, dev)
        three = pose.launch_refine_joint(in_dev, edgels, Kd, three_view=True)
        buf = _sentinel(E, dev)
        full = pose.launch_refine_joint(in_dev, edgels, Kd, structure=True, tangents=tangents[:E], edgels3d=buf)
        assert [_bytes(a) for a in full[:5] if a is not None] == [_bytes(a) for a in three if a is not None], name
        rep = pose.structure_report_dict(full[6])
        assert rep == dict(status=_abi.HC_STRUCTURE_NONE, none=True, count=0, tangents=0, oriented=0,
                           scale31=np.float32(s["scale31"])), name
        assert G.is_poisoned(buf), name
        assert pose.three_view_report_dict(full[4])["skipped"], name
        # structure-only: NONE without a path alone; with one the rule runs on the input's own scale
        buf = _sentinel(E, dev)
        out, rec_dev, srep = pose.launch_reconstruct(in_dev, edgels, tangents[:E], Kd, edgels3d=buf)
        rep = pose.structure_report_dict(srep)
        assert _bytes(out) == _bytes(in_dev), name
        if name == "none":
            assert rep["none"] and rep["count"] == 0 and G.is_poisoned(buf)
        else:
            _against_reference("far, structure only", pose.structure_records(rec_dev, rep), rep, s, far,
                               ransac0.tangents[:65], K)
            assert rep["status"] == 0 and G.is_poisoned(buf[rep["count"] * 48:])
    best, rank, _, reps, srep, rec = pose.refine_topk([none, none], scenes["clean"]["dev"][:257], Kd, structure=True,
                                                      tangents=tangents[:257])
    assert rank == -1 and best["path"] == -1 and srep["none"] and srep["count"] == 0 and len(rec) == 0


# ---- graph capture and replay -------------------------------------------------------------------------

def test_graph_replay_of_the_four_stages(scenes):
    """launch_refine_joint(structure=True) and launch_reconstruct recorded once
    and replayed twice: both replays give the eager call's bytes, with every
    output poisoned from outside the graph before each replay (the records
    beyond count then still are)."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    sel, edgels, tangents, K, _, _ = _case(scenes, "noisy", 2049)
    dev = edgels.device
    in_dev = _upload(sel, dev)
    buf = _sentinel(2049, dev)

    def full():
        return pose.launch_refine_joint(in_dev, edgels, K, structure=True, tangents=tangents, transfer_mask=True,
                                        edgels3d=buf)

    def only():
        return pose.launch_reconstruct(in_dev, edgels, tangents, K, edgels3d=buf)
    for enqueue in (full, only):
        G.poison(buf)
        eager = [_bytes(t) for t in enqueue()]
        count = pose.structure_report_dict(np.frombuffer(eager[-1], np.uint8))["count"]
        assert 0 < count < 2049
        cap, out = G.capture(enqueue)
        try:
            for _ in range(2):
                G.poison(*out)
                cap.replay()
                torch.cuda.synchronize()
                assert [_bytes(t) for t in out] == eager
                assert G.is_poisoned(buf[count * 48:])
        finally:
            G.release(cap)
