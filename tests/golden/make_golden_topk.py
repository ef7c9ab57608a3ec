"""Generates tests/golden/pose_topk_noisy1px_trial12_N100.npz from the C oracle on the CPU.

Trial 12 of the config-5 protocol (Triplet_Edgels_000 with sigma = 1 px noise,
noise seed 20250215 + 12, samples srand(12), 100 samples): the run whose joint
winner sits in a wrong basin, while the candidate ranked third refines to the
right pose.  Its candidate paths, their joint counts (tests/joint_reference.py:
the unmodified oracle on one-edgel scenes) and the numpy reference of the top-k
calls (tests/topk_reference.py) for ranks 0..7:

  trial, noise_seed
  cand_ids (35,) int32, cand_tracks (35, 31, 2) float32
  counts   (35, 3) int32     (joint, inliers21, inliers31) per candidate
  ranking  (35,) int32       indices into cand_ids, by descending key joint << 32 | id
  in_pose, ref_pose (8, 24) float32   R21 | t21 | R31 | t31 of rank r as the oracle converts its
                             track, and as refine_reference.refine returns it
  ref_counts (8, 3) int32    the refined pose's (joint, 21, 31)
  ref_history (8, 33) int32, ref_status, ref_best_iteration (8,) int32
  ok_before, ok_after (8,) bool, res_before, res_after (8, 4) float32   the GT verdict
  borderline (8,) int32      edgels within 0.01 px of the gate under the refined pose
  best_rank_k4               the rank the reference selects among ranks 0..3

The script asserts what tests/test_gpu_topk.py relies on and fails otherwise.

Run:  python tests/golden/make_golden_topk.py      (a few minutes)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import refine_reference as RR  # noqa: E402
import topk_reference as TR  # noqa: E402
from joint_reference import joint_reference  # noqa: E402
from make_golden import NOISE_SEED, PROB, RANS  # noqa: E402
from oracle import oracle as O  # noqa: E402

TRIAL, RANKS = 12, 8


def flat(p):
    return np.concatenate([np.asarray(p[k], np.float32).reshape(-1) for k in RR.POSE_KEYS])


def main():
    ss, sp, dhdx, dhdt = O.read_problem(PROB)
    U = np.concatenate([dhdx, dhdt]).astype(np.int32)
    loc, tan = O.read_edgels(os.path.join(RANS, "Triplet_Edgels", "Triplet_Edgels_000.txt"))
    K = O.read_floats(os.path.join(RANS, "Intrinsic_Matrix.txt"), 9)
    gt21 = O.read_floats(os.path.join(RANS, "GT_Poses21", "GT_Poses21_000.txt"), 12)
    gt31 = O.read_floats(os.path.join(RANS, "GT_Poses31", "GT_Poses31_000.txt"), 12)
    nloc = O.add_pixel_noise(loc, K, 1.0, NOISE_SEED + TRIAL)
    tgt, dif, _ = O.prepare_target_params(TRIAL, [100], nloc, tan, sp)
    tr, conv, _, _ = O.gpuhc_track(ss, sp, tgt, dif, U)
    inl, _ = O.pose_support(tr, conv, nloc, K)
    ids = np.nonzero(inl[:, 0] >= 0)[0].astype(np.int32)
    ref = joint_reference(O, tr[ids], nloc, K, ids)
    assert ref["cand"].all() and np.array_equal(ref["counts"][:, 1:], inl[ids])
    counts = ref["counts"]
    ranking = np.array(TR.rank(counts, ids), np.int32)
    assert len(ids) == 35 and len(ranking) == 35
    assert ids[ranking[:4]].tolist() == [29311, 15336, 3607, 20328]
    assert counts[ranking[:8], 0].tolist() == [644, 605, 574, 563, 410, 390, 249, 245]
    assert ids[ranking[0]] == ref["path"]                     # rank 0 is the joint call's winner

    one = np.ones(1, np.uint8)
    poses = []
    for i in ranking[:RANKS]:
        _, s = O.pose_support(tr[ids[i]:ids[i] + 1], one, nloc[:0], K)
        p = {k: np.asarray(s[k], np.float32) for k in RR.POSE_KEYS}
        m21, m31 = RR.score(nloc, K, tuple(p[k] for k in RR.POSE_KEYS))
        assert [int((m21 & m31).sum()), int(m21.sum()), int(m31.sum())] == counts[i].tolist()
        poses.append(p)
    refined, best8 = TR.refine_topk(poses, ids[ranking[:RANKS]], nloc, K)
    _, best4 = TR.refine_topk(poses[:4], ids[ranking[:4]], nloc, K)
    before = [O.pose_residuals(gt21, gt31, p) for p in poses]
    after = [O.pose_residuals(gt21, gt31, {k: r[k] for k in RR.POSE_KEYS}) for r in refined]
    B = np.array([RR.borderline(nloc, K, r["pose64"]) for r in refined], np.int32)
    rc = np.array([[r["inliers"], r["inliers21"], r["inliers31"]] for r in refined], np.int32)

    # what the repair test relies on
    assert best4 == 2 and rc[:4, 0].tolist() == [644, 605, 3603, 563]
    assert not before[0][1] and not after[0][1] and not before[2][1] and after[2][1]
    assert rc[2, 0] - max(rc[0, 0], rc[1, 0], rc[3, 0]) > 10 * max(1, int(B[:4].max())), B[:4]
    assert max(after[2][0][0], after[2][0][1]) < 0.02                       # rad, the gate is 0.1
    assert [r for r in range(RANKS) if after[r][1]] == [2, 4, 6]

    np.savez_compressed(
        os.path.join(HERE, "pose_topk_noisy1px_trial12_N100.npz"), trial=np.int32(TRIAL),
        noise_seed=np.int64(NOISE_SEED + TRIAL), cand_ids=ids, cand_tracks=tr[ids], counts=counts, ranking=ranking,
        in_pose=np.stack([flat(p) for p in poses]), ref_pose=np.stack([flat(r) for r in refined]), ref_counts=rc,
        ref_history=np.stack([r["joint_history"] for r in refined]).astype(np.int32),
        ref_status=np.array([r["status"] for r in refined], np.int32),
        ref_best_iteration=np.array([r["best_iteration"] for r in refined], np.int32),
        ok_before=np.array([b[1] for b in before], bool), ok_after=np.array([a[1] for a in after], bool),
        res_before=np.stack([b[0] for b in before]).astype(np.float32),
        res_after=np.stack([a[0] for a in after]).astype(np.float32), borderline=B, best_rank_k4=np.int32(best4),
        best_rank_k8=np.int32(best8))
    print("top-k noisy 1px trial 12: candidates", len(ids), "ranks 0..7 at", ids[ranking[:RANKS]].tolist(), "refined",
          rc[:, 0].tolist(), "ok", [bool(a[1]) for a in after], "borderline", B.tolist(), "best of 4:", best4,
          "best of 8:", best8)


if __name__ == "__main__":
    main()
