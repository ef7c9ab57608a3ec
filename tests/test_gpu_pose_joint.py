"""GPU tests of the joint pose selection (hc_trifocal_pose_support_joint, its
grouped form, hc_trifocal_pose_inlier_mask, hc_pose_merge_joint, and the
solver's Pose_Selection_Joint setting through the CLI).

Expected values come from the unmodified oracle (tests/joint_reference.py: one
oracle call per edgel gives every candidate's per-view inlier masks), pose bits
from hc_trifocal_pose_support with only the selected path converged.  The
per-view call, which shares the joint call's edgel loop, is checked against the
same masks at the same remainder sizes.

Common inputs: the 36 candidate tracks of pose_N100_seed0.npz at scattered batch
ids of a 624-path buffer whose other paths are not converged; the scene is the
first E edgels of dataset 000 with sigma = 1 px noise (seed 20250215), so that
inlier-ness differs per edgel and per view.
"""
import numpy as np
import pytest

from checks import golden, noisy_data, run_cli
from joint_reference import joint_reference, pack_mask

pytestmark = pytest.mark.gpu

NPATHS = 624
SIZES = [1, 63, 64, 65, 200]
POSE_KEYS = ("R21", "t21", "R31", "t31")


def _empty_tracks(n):
    tr = np.zeros((n, 31, 2), np.float32)
    tr[:, 30, 0] = 1.0
    return tr, np.zeros(n, np.uint8)


@pytest.fixture(scope="module")
def noisy0():
    return noisy_data()


@pytest.fixture(scope="module")
def common(oracle, noisy0):
    """Tracks, ids, and the oracle's per-edgel masks over the first 200 edgels
    (computed once; the reference of a smaller E is their first E columns)."""
    g = golden("pose_N100_seed0")
    cand = np.ascontiguousarray(g["cand_tracks"])
    rng = np.random.default_rng(11)
    ids = np.sort(rng.choice(NPATHS, len(cand), replace=False))
    assert (ids < 312).sum() >= 8 and (ids >= 312).sum() >= 8
    tr, conv = _empty_tracks(NPATHS)
    tr[ids] = cand
    conv[ids] = 1
    ref = joint_reference(oracle, cand, noisy0.locations[:200], noisy0.K, ids)
    for v in (tr, conv, ids, ref["m21"], ref["m31"]):
        v.setflags(write=False)
    return dict(cand=cand, ids=ids, tracks=tr, conv=conv, m21=ref["m21"], m31=ref["m31"])


def _reference(common, E, rows=None):
    """The joint reference over the first E edgels for the candidates `rows`
    (indices into common['cand'], default all), from the shared masks."""
    rows = np.arange(len(common["ids"])) if rows is None else np.asarray(rows)
    m21, m31 = common["m21"][rows, :E], common["m31"][rows, :E]
    mJ = m21 & m31
    counts = np.stack([mJ.sum(1), m21.sum(1), m31.sum(1)], axis=1).astype(np.int32)
    w = -1
    for i in range(len(rows)):
        if w < 0 or counts[i, 0] >= counts[w, 0]:
            w = i
    return dict(counts=counts, winner=w, mask=mJ[w] if w >= 0 else np.zeros(E, bool))


@pytest.fixture(scope="module")
def dev_inputs(tracker, common, noisy0):
    import torch
    dev = tracker.device
    return dict(tracks=torch.from_numpy(common["tracks"].copy()).to(dev),
                conv=torch.from_numpy(common["conv"].copy()).to(dev),
                edgels=torch.from_numpy(np.array(noisy0.locations[:200])).to(dev),
                K=torch.from_numpy(np.ascontiguousarray(noisy0.K)).to(dev))


def _scale31(track):
    """|Re x[21..23]| / |Re x[18..20]| in float32, the summation order of unit3."""
    x = track[18:24, 0].astype(np.float32)
    n21 = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    n31 = np.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
    assert n21.dtype == np.float32
    return n31 / n21


def _assert_none(sel):
    assert (sel["num_candidates"], sel["path"], sel["inliers"], sel["inliers21"], sel["inliers31"], sel["key"]) == \
        (0, -1, -1, -1, -1, 0)
    assert not any(sel[k].any() for k in POSE_KEYS) and sel["scale31"] == 0


def _pose_of_path(d, path, E):
    """hc_trifocal_pose_support with only `path` converged."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    only = torch.zeros_like(d["conv"])
    only[path] = 1
    _, s = pose.pose_support(d["tracks"], only, d["edgels"][:E], d["K"])
    assert s["path21"] == s["path31"] == path
    return s


@pytest.mark.parametrize("E", SIZES)
def test_joint_single_triplet_and_mask(common, dev_inputs, E):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = dev_inputs
    ids = common["ids"]
    ref = _reference(common, E)
    inl, sel, sel_dev = pose.pose_support_joint(d["tracks"], d["conv"], d["edgels"][:E], d["K"],
                                                return_device_selection=True)
    assert inl.shape == (NPATHS, 3)
    assert np.array_equal(inl[ids], ref["counts"]), np.nonzero((inl[ids] != ref["counts"]).any(1))[0]
    other = np.ones(NPATHS, bool)
    other[ids] = False
    assert (inl[other] == -1).all()
    w = ref["winner"]
    path = int(ids[w])
    assert sel["num_candidates"] == len(ids)
    assert (sel["path"], sel["inliers"], sel["inliers21"], sel["inliers31"]) == (path, *ref["counts"][w].tolist())
    assert sel["key"] == (int(ref["counts"][w, 0]) << 32) | path
    one = _pose_of_path(d, path, E)
    for k in POSE_KEYS:
        assert sel[k].tobytes() == one[k].tobytes(), k
    exp = _scale31(common["tracks"][path])
    assert sel["scale31"].tobytes() == np.float32(exp).tobytes(), (sel["scale31"], exp)
    # mask of the device-resident selection
    words = pose.inlier_mask(sel_dev, d["edgels"][:E], d["K"], packed=True)
    assert words.dtype == np.uint64 and words.shape == ((E + 63) // 64,)
    assert np.array_equal(words, pack_mask(ref["mask"]))          # bits at or beyond E are 0
    assert sum(bin(int(v)).count("1") for v in words) == sel["inliers"]
    mask = pose.inlier_mask(sel_dev, d["edgels"][:E], d["K"])
    assert mask.dtype == bool and mask.shape == (E,) and np.array_equal(mask, ref["mask"])


@pytest.mark.parametrize("E", SIZES)
def test_per_view_counts_at_remainder_sizes(common, dev_inputs, E):
    """hc_trifocal_pose_support runs the edgel loop it shares with the joint
    call: its counts and per-view winners over the first E edgels against the
    oracle's masks alone."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = dev_inputs
    ids = common["ids"]
    counts = np.stack([common["m21"][:, :E].sum(1), common["m31"][:, :E].sum(1)], axis=1).astype(np.int32)
    inl, sel = pose.pose_support(d["tracks"], d["conv"], d["edgels"][:E], d["K"])
    assert inl.shape == (NPATHS, 2)
    assert np.array_equal(inl[ids], counts), np.nonzero((inl[ids] != counts).any(1))[0]
    other = np.ones(NPATHS, bool)
    other[ids] = False
    assert (inl[other] == -1).all()
    assert sel["num_candidates"] == len(ids) == 36
    for v, view in enumerate(("21", "31")):
        c = counts[:, v]
        w = int(np.nonzero(c == c.max())[0][-1])    # ids ascend: the last candidate attaining the maximum
        path = int(ids[w])
        assert (sel["path" + view], sel["inliers" + view]) == (path, int(c[w])), view
        assert sel["key" + view] == (int(c[w]) << 32) | path, view


def test_joint_tie_selects_the_larger_batch_id(common, dev_inputs):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = dev_inputs
    tr, conv = _empty_tracks(NPATHS)
    tr[100] = tr[500] = common["cand"][0]
    conv[[100, 500]] = 1
    inl, sel = pose.pose_support_joint(torch.from_numpy(tr).to(d["tracks"].device),
                                       torch.from_numpy(conv).to(d["tracks"].device), d["edgels"], d["K"])
    assert sel["num_candidates"] == 2 and (inl[100] == inl[500]).all() and inl[500, 0] >= 0
    assert sel["path"] == 500 and sel["key"] == (int(inl[500, 0]) << 32) | 500


def test_joint_without_candidates(dev_inputs):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = dev_inputs
    inl, sel, sel_dev = pose.pose_support_joint(d["tracks"], torch.zeros_like(d["conv"]), d["edgels"], d["K"],
                                                return_device_selection=True)
    assert (inl == -1).all()
    _assert_none(sel)
    words = pose.inlier_mask(sel_dev, d["edgels"], d["K"], packed=True)
    assert words.shape == (4,) and not words.any()
    inl, sel = pose.pose_support_joint(d["tracks"][:0], d["conv"][:0], d["edgels"], d["K"])
    assert inl.shape == (0, 3)
    _assert_none(sel)


def test_joint_grouped(problem, tracker, common, noisy0, ransac0):
    """Triplets 0 (E = 63) and 1 (E = 200, another noise seed) with interleaved
    samples and a third triplet whose one sample has no candidate: each
    selection is the single-triplet joint call over that triplet's own rows."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    other = noisy_data(20250216)
    batch = TripletBatch(problem, [noisy0, other, ransac0], seeds=0, samples_per_triplet=[2, 2, 1], interleave=True,
                         edgel_counts=[63, 200, 100])
    assert batch.sample_group.tolist() == [0, 1, 2, 0, 1]
    db = batch.to(tracker.device)
    n = 5 * 312
    tr, conv = _empty_tracks(n)
    rng = np.random.default_rng(12)
    spots = np.sort(rng.choice(np.setdiff1d(np.arange(n), np.arange(624, 936)), 72, replace=False))
    tr[spots] = np.concatenate([common["cand"], common["cand"]])[rng.permutation(72)]
    conv[spots] = 1
    T = torch.from_numpy(tr).to(tracker.device)
    Cv = torch.from_numpy(conv).to(tracker.device)
    inl, sels = pose.pose_support_joint_grouped(T, Cv, db)
    assert inl.shape == (n, 3) and len(sels) == 3
    for t in range(2):
        rows = batch.path_index(t)
        assert conv[rows].sum() >= 8
        idx = torch.from_numpy(rows).to(tracker.device)
        inl_r, ref = pose.pose_support_joint(T[idx].contiguous(), Cv[idx].contiguous(), db.group_edgels(t), db.K[t])
        assert np.array_equal(inl[rows], inl_r), t
        assert ref["path"] >= 0
        for k in ("num_candidates", "inliers", "inliers21", "inliers31"):
            assert sels[t][k] == ref[k], (t, k)
        assert sels[t]["path"] == int(rows[ref["path"]])
        assert sels[t]["key"] == (ref["inliers"] << 32) | int(rows[ref["path"]])
        for k in POSE_KEYS + ("scale31",):
            assert sels[t][k].tobytes() == ref[k].tobytes(), (t, k)
    assert (inl[624:936] == -1).all()
    _assert_none(sels[2])


def test_joint_merge_of_two_launches(common, dev_inputs):
    """The 624 paths in two calls, merged on the host: the one-call selection,
    and the uploaded merged selection gives the one-call mask."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = dev_inputs
    _, full, full_dev = pose.pose_support_joint(d["tracks"], d["conv"], d["edgels"], d["K"],
                                                return_device_selection=True)
    mask = pose.inlier_mask(full_dev, d["edgels"], d["K"])
    for cut in (312, 0):
        parts = [pose.pose_support_joint(d["tracks"][a:b], d["conv"][a:b], d["edgels"], d["K"])[1]
                 for a, b in ((0, cut), (cut, NPATHS))]
        m = pose.merge_joint(parts, [0, cut])
        for k in ("num_candidates", "path", "inliers", "inliers21", "inliers31", "key"):
            assert m[k] == full[k], k
        for k in POSE_KEYS + ("scale31",):
            assert m[k].tobytes() == full[k].tobytes(), k
        assert np.array_equal(pose.inlier_mask(m, d["edgels"], d["K"]), mask)
    assert mask.sum() == full["inliers"]


def test_joint_marginal_counts_at_n100(samples100, tracker):
    """One tracked config-2 launch, all 5117 edgels: the joint call's per-view
    counts are hc_trifocal_pose_support's, for every path."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    tgt, dif, _ = samples100
    r = tracker.track(tgt, dif)
    inl2, _ = pose.pose_support(r.tracks, r.converge, tracker.edgels, tracker.K)
    inl3, sel = pose.pose_support_joint(r.tracks, r.converge, tracker.edgels, tracker.K)
    assert inl3.shape == (31200, 3) and np.array_equal(inl3[:, 1:], inl2)
    assert ((inl3[:, 0] >= 0) == (inl2[:, 0] >= 0)).all() and (inl3[:, 0] <= inl3[:, 1:].min(1)).all()
    assert sel["num_candidates"] == int((inl2[:, 0] >= 0).sum()) > 0
    assert [sel["inliers"], sel["inliers21"], sel["inliers31"]] == inl3[sel["path"]].tolist()
    assert sel["inliers"] == inl3[:, 0].max()


def test_joint_noisy_golden(tracker, noisy0):
    """The config-5 fixture's 31 candidates over all 5117 noisy edgels against
    pose_joint_noisy1px_N100.npz (the oracle on the CPU): counts, winner, mask."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    g = golden("pose_joint_noisy1px_N100")
    ids = g["cand_ids"]
    assert len(ids) == 31
    tr, conv = _empty_tracks(31200)
    tr[ids] = g["cand_tracks"]
    conv[ids] = 1
    dev = tracker.device
    edgels = torch.from_numpy(np.array(noisy0.locations)).to(dev)
    K = torch.from_numpy(np.ascontiguousarray(noisy0.K)).to(dev)
    assert edgels.shape[0] == 5117
    inl, sel, sel_dev = pose.pose_support_joint(torch.from_numpy(tr).to(dev), torch.from_numpy(conv).to(dev), edgels, K,
                                                return_device_selection=True)
    assert np.array_equal(inl[ids], g["counts"])
    assert sel["num_candidates"] == 31 and sel["path"] == int(g["path"]) and sel["key"] == int(g["key"])
    assert [sel["inliers"], sel["inliers21"], sel["inliers31"]] == g["inliers"].tolist()
    words = pose.inlier_mask(sel_dev, edgels, K, packed=True)
    assert np.array_equal(words, g["mask"])
    assert sum(bin(int(v)).count("1") for v in words) == sel["inliers"]


def test_cli_joint_option(tmp_path, samples100, tracker):
    """`magmaHC-main --joint` (setting Pose_Selection_Joint) on config 2: the
    solver selects the path the joint call selects on the same launch, for both
    views, prints the joint count and still recovers the GT pose."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    tgt, dif, _ = samples100
    r = tracker.track(tgt, dif)
    _, sel = pose.pose_support_joint(r.tracks, r.converge, tracker.edgels, tracker.K)
    stdout, read = run_cli(tmp_path, "--joint")
    assert f" - joint selection: path {sel['path']}, {sel['inliers']} edgels within 2 px in both views" in stdout
    pr = read("GPU_Pose_Results.txt").split()
    assert int(pr[0]) == 1 and int(pr[5]) == int(pr[6]) == sel["path"] and int(pr[7]) == sel["num_candidates"]
    assert max(float(v) for v in pr[1:5]) < 1e-3
