"""Generates tests/golden/pose_joint_noisy1px_N100.npz from the C oracle on the CPU.

The config-5 fixture of make_golden.py (Triplet_Edgels_000 with sigma = 1 px
noise, noise seed 20250215, samples srand(0), 100 samples): its candidate paths'
ids and tracks, and the joint selection's reference over all 5117 noisy edgels
(tests/joint_reference.py: the unmodified oracle on one-edgel scenes):

  cand_ids (31,) int32, cand_tracks (31, 31, 2) float32
  counts   (31, 3) int32   (joint, inliers21, inliers31) per candidate
  path, inliers (3,), key  the winner: batch id, its three counts, count << 32 | id
  mask     (80,) uint64    the winner's packed joint inlier mask

Run:  python tests/golden/make_golden_joint.py      (about a minute)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from joint_reference import joint_reference, pack_mask  # noqa: E402
from make_golden import NOISE_SEED, PROB, RANS  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    ss, sp, dhdx, dhdt = O.read_problem(PROB)
    U = np.concatenate([dhdx, dhdt]).astype(np.int32)
    loc, tan = O.read_edgels(os.path.join(RANS, "Triplet_Edgels", "Triplet_Edgels_000.txt"))
    K = O.read_floats(os.path.join(RANS, "Intrinsic_Matrix.txt"), 9)
    nloc = O.add_pixel_noise(loc, K, 1.0, NOISE_SEED)
    tgt, dif, _ = O.prepare_target_params(0, [100], nloc, tan, sp)
    tr, conv, _, _ = O.gpuhc_track(ss, sp, tgt, dif, U)
    inl, _ = O.pose_support(tr, conv, nloc, K)
    ids = np.nonzero(inl[:, 0] >= 0)[0].astype(np.int32)
    # the same candidates and marginal counts as the committed config-5 fixture
    old = np.load(os.path.join(HERE, "gpuhc_noisy1px_N100.npz"))
    assert len(ids) == int(old["num_candidates"]) and np.array_equal(inl[ids], old["cand_inliers"])
    ref = joint_reference(O, tr[ids], nloc, K, ids)
    assert ref["cand"].all() and np.array_equal(ref["counts"][:, 1:], inl[ids])
    w = ref["winner"]
    np.savez_compressed(os.path.join(HERE, "pose_joint_noisy1px_N100.npz"), cand_ids=ids, cand_tracks=tr[ids],
                        counts=ref["counts"], path=np.int32(ref["path"]), inliers=ref["counts"][w],
                        key=np.uint64(ref["key"]), mask=pack_mask(ref["mask"]))
    print("joint noisy 1px: candidates", len(ids), "winner", ref["path"], "counts (joint, 21, 31)",
          ref["counts"][w].tolist())


if __name__ == "__main__":
    main()
