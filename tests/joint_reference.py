"""Reference of the joint pose selection, from the unmodified oracle.

oracle.pose_support over a ONE-edgel scene returns, per candidate, whether that
edgel is an inlier in view 1-2 and in view 1-3 (its count is 0 or 1).  Looping
over the edgels gives the two masks of every candidate, their AND, all three
counts and the expected winner (most joint inliers, ties -> the last one).
"""
import numpy as np


def edgel_masks(oracle, tracks, loc, K):
    """tracks (n, 31, 2), all treated as converged.  Returns (cand (n,) bool,
    m21, m31 (n, E) bool): candidate flags and the per-view inlier masks
    (all False for a non-candidate)."""
    tracks = np.ascontiguousarray(tracks, np.float32)
    loc = np.ascontiguousarray(loc, np.float32)
    n, E = tracks.shape[0], loc.shape[0]
    ones = np.ones(n, np.uint8)
    cand = oracle.pose_support(tracks, ones, loc[:0], K)[0][:, 0] >= 0
    m21 = np.zeros((n, E), bool)
    m31 = np.zeros((n, E), bool)
    for e in range(E):
        inl, _ = oracle.pose_support(tracks, ones, loc[e:e + 1], K)
        assert ((inl >= 0).all(axis=1) == cand).all() and inl.max(initial=0) <= 1
        m21[:, e] = inl[:, 0] == 1
        m31[:, e] = inl[:, 1] == 1
    return cand, m21, m31


def joint_reference(oracle, tracks, loc, K, ids=None):
    """The expected result of the joint call over `tracks` placed at batch ids
    `ids` (default 0..n-1, ascending): dict with cand, m21, m31, mJ, counts
    (n, 3) int32 = (joint, 21, 31) with -1 for non-candidates, winner (index into
    tracks, -1: none), path (its batch id), key, mask (the winner's AND-mask,
    all False without a winner)."""
    cand, m21, m31 = edgel_masks(oracle, tracks, loc, K)
    n, E = m21.shape
    ids = np.arange(n) if ids is None else np.asarray(ids)
    assert (np.diff(ids) > 0).all()
    mJ = m21 & m31
    counts = np.stack([mJ.sum(1), m21.sum(1), m31.sum(1)], axis=1).astype(np.int32)
    counts[~cand] = -1
    winner = -1
    for i in range(n):   # >= : the last candidate attaining the maximum
        if cand[i] and (winner < 0 or counts[i, 0] >= counts[winner, 0]):
            winner = i
    path = int(ids[winner]) if winner >= 0 else -1
    key = (int(counts[winner, 0]) << 32) | path if winner >= 0 else 0
    mask = mJ[winner] if winner >= 0 else np.zeros(E, bool)
    return dict(cand=cand, m21=m21, m31=m31, mJ=mJ, counts=counts, winner=winner, path=path, key=key, mask=mask)


def pack_mask(mask):
    """bool (E,) -> (E + 63) // 64 uint64 words, bit e % 64 of word e // 64."""
    E = len(mask)
    b = np.zeros(((E + 63) // 64) * 64, np.uint8)
    b[:E] = mask
    return np.packbits(b, bitorder="little").view(np.uint64)
