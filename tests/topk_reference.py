"""Reference of the top-k calls (include/topk/hc_pose_topk.h), in numpy only:
the ranking of the candidates by key, the refinement of the k best
(tests/refine_reference.py) and the selection among the refined ones.
"""
import numpy as np

import refine_reference as RR


def keys(counts, ids=None):
    """counts (n, 3) int (joint, 21, 31; joint < 0: no candidate), ids (n,) batch
    ids (default 0..n-1) -> (n,) Python ints joint << 32 | id, -1 for non-candidates."""
    counts = np.asarray(counts)
    ids = np.arange(len(counts)) if ids is None else np.asarray(ids)
    return [(int(c) << 32) | int(b) if c >= 0 else -1 for c, b in zip(counts[:, 0], ids)]


def rank(counts, ids=None, k=None):
    """Indices into counts of the candidates, by descending key (most joint
    inliers, ties -> the larger batch id); the first k of them with k."""
    ky = keys(counts, ids)
    order = sorted((i for i in range(len(ky)) if ky[i] >= 0), key=lambda i: -ky[i])
    return order if k is None else order[:k]


def refine_topk(poses, paths, loc, K, iterations=10, min_inliers=16):
    """poses: the ranked candidates' poses (dicts with R21, t21, R31, t31), None
    for a "none" rank; paths: their batch ids.  Returns (refined, best_rank):
    refine_reference.refine of every pose (None for none) and the rank with the
    largest inliers << 32 | path, -1 without a candidate."""
    refined = [None if p is None else RR.refine(p, loc, K, iterations, min_inliers) for p in poses]
    best, best_key = -1, -1
    for r, (ref, path) in enumerate(zip(refined, paths)):
        if ref is None:
            continue
        key = (int(ref["inliers"]) << 32) | int(path)
        if key > best_key:
            best, best_key = r, key
    return refined, best
