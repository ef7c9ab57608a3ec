"""CPU tests of the grouped (multi-triplet) launches' host side: the group
validation every grouped launch goes through, the argument checks of the two C
entry points (made before any device work) and the sample layout of
multi.TripletBatch against per-triplet prepare_target_params."""
import ctypes as C

import numpy as np
import pytest


def test_check_groups_accepts_a_valid_grouping():
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import check_groups
    check_groups(np.array([0, 1, 2, 2, 0], np.int32), 3, 5, [5117, 1000, 1])
    check_groups(np.array([0, 0], np.int64), 1, 2, np.array([7]))
    check_groups(np.zeros(0, np.int32), 2, 0, [3, 4])


@pytest.mark.parametrize("sample_group,num_groups,num_samples,edgel_counts", [
    ([0, 1, 1], 2, 4, [10, 10]),           # wrong length
    ([[0, 1], [1, 0]], 2, 4, [10, 10]),    # not one id per sample
    ([0, -1, 1], 2, 3, [10, 10]),          # id -1
    ([0, 2, 1], 2, 3, [10, 10]),           # id T
    ([0, 1, 1], 2, 3, [10, 0]),            # zero edgel count
    ([0, 1, 1], 2, 3, [10, -4]),           # negative edgel count
    ([0, 0, 0], 2, 3, [10]),               # one count per group
    ([0, 0, 0], 0, 3, []),                 # no groups
])
def test_check_groups_rejects(sample_group, num_groups, num_samples, edgel_counts):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import check_groups
    with pytest.raises(_abi.HCError):
        check_groups(np.array(sample_group, np.int32), num_groups, num_samples, edgel_counts)


def test_struct_layouts():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, multi
    assert C.sizeof(_abi.hcTripletGroup) == 24 == multi.GROUP_DTYPE.itemsize
    assert [(_abi.hcTripletGroup.locations.offset, _abi.hcTripletGroup.K.offset,
             _abi.hcTripletGroup.num_edgels.offset)] == [(0, 8, 16)]
    assert [multi.GROUP_DTYPE.fields[k][1] for k in ("locations", "K", "num_edgels", "pad")] == [0, 8, 16, 20]
    g = _abi.hcGroupedAbortArgs
    assert (g.num_groups.offset, g.groups.offset, g.sample_group.offset, g.group_found.offset,
            g.trifocal_sols_batch_index.offset, g.group_found_ticks.offset, g.inflight_stop.offset) == \
        (0, 8, 16, 24, 32, 40, 48)
    assert _abi.lib().hc_trifocal_abi_version() == 2   # additive: no existing struct changed


def test_grouped_abort_rejects_bad_arguments_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    ws = int(L.hc_trifocal_workspace_size())
    dummy = C.c_void_p(0x1000)          # never dereferenced: validation fails first
    a = _abi.hcTrackArgs()
    a.sub_ransac_iters = 1
    a.settings = _abi.hcTrackSettings(80, 3, 4)
    for f in ("start_sols", "tracks", "start_params", "target_params", "diff_params", "unified_index",
              "converge", "infinity"):
        setattr(a, f, 0x1000)
    fn = L.hc_trifocal_2op1p_30x30_track_abort_grouped

    def args(**kw):
        g = _abi.hcGroupedAbortArgs()
        g.num_groups = 2
        for f in ("groups", "sample_group", "group_found", "trifocal_sols_batch_index"):
            setattr(g, f, 0x1000)
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    assert fn(C.byref(a), None, dummy, ws, None) == 1
    assert fn(None, C.byref(args()), dummy, ws, None) == 1
    assert fn(C.byref(a), C.byref(args(groups=None)), dummy, ws, None) == 1          # null descriptor array
    assert fn(C.byref(a), C.byref(args(num_groups=0)), dummy, ws, None) == 1
    assert fn(C.byref(a), C.byref(args(num_groups=-3)), dummy, ws, None) == 1
    for f in ("sample_group", "group_found", "trifocal_sols_batch_index"):
        assert fn(C.byref(a), C.byref(args(**{f: None})), dummy, ws, None) == 1, f
    # the group checks come first; then the single launch's own (workspace, sizes)
    assert fn(C.byref(a), C.byref(args()), None, ws, None) == 2
    assert fn(C.byref(a), C.byref(args()), dummy, ws - 1, None) == 2
    a.sub_ransac_iters = 0               # zero samples: a no-op success, ticks optional
    assert fn(C.byref(a), C.byref(args(group_found_ticks=None)), dummy, ws, None) == 0


def test_grouped_pose_rejects_bad_arguments_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    fn = _abi.lib().hc_trifocal_pose_support_grouped
    d = C.c_void_p(0x1000)
    assert fn(312, d, d, 2, None, d, 0, d, d, None) == 1                              # null descriptor array
    assert fn(312, d, d, 0, d, d, 0, d, d, None) == 1                                 # num_groups = 0
    assert fn(312, d, d, 2, d, d, _abi.HC_POSE_REFERENCE_QUIRKS, d, d, None) == 1     # the quirks flag
    assert fn(312, d, d, 2, d, None, 0, d, d, None) == 1                              # null sample_group
    assert fn(312, d, d, 2, d, d, 0, d, None, None) == 1                              # null selections
    assert fn(-312, d, d, 2, d, d, 0, d, d, None) == 1
    assert fn(100, d, d, 2, d, d, 0, d, d, None) == 1                                 # not whole samples


@pytest.fixture(scope="module")
def three(problem):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data, prepare_target_params
    datas = [load_ransac_data(i) for i in (0, 50, 99)]
    counts = [5, 3, 4]
    per = [prepare_target_params(problem, d, seed=0, num_samples=c) for d, c in zip(datas, counts)]
    return datas, counts, per


@pytest.mark.parametrize("interleave", [False, True])
def test_triplet_batch_rows_and_groups(problem, three, interleave):
    """Rows equal per-triplet prepare_target_params in both orders; sample_group,
    the per-triplet index lists and the scoring sets are right."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    datas, counts, per = three
    b = TripletBatch(problem, datas, seeds=0, samples_per_triplet=counts, interleave=interleave,
                     edgel_counts=[None, 1000, 777])
    assert b.num_groups == 3 and b.num_samples == 12
    assert b.target.shape == (12, 34, 2) and b.diff.shape == (12, 34, 2) and b.sample_group.dtype == np.int32
    if interleave:   # round-robin while a triplet has samples left
        expect = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 2, 0]
    else:
        expect = [0] * 5 + [1] * 3 + [2] * 4
    assert b.sample_group.tolist() == expect
    for t in range(3):
        assert b.index[t].tolist() == [i for i, g in enumerate(expect) if g == t]
        assert np.array_equal(b.target[b.index[t]], per[t][0])
        assert np.array_equal(b.diff[b.index[t]], per[t][1])
        assert np.array_equal(b.picked[b.index[t]], per[t][2])
        assert np.array_equal(b.path_index(t)[:313], np.r_[b.index[t][0] * 312 + np.arange(312),
                                                            b.index[t][1] * 312])
    assert b.edgel_counts.tolist() == [5117, 1000, 777]
    assert np.array_equal(b.locations[1], datas[1].locations[:1000])
    assert np.array_equal(b.locations[2], datas[2].locations[:777])


def test_triplet_batch_rejects_bad_input(problem, three):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    datas, _, _ = three
    with pytest.raises(_abi.HCError):
        TripletBatch(problem, [], samples_per_triplet=1)
    with pytest.raises(_abi.HCError):
        TripletBatch(problem, datas, samples_per_triplet=[1, 2])
    with pytest.raises(_abi.HCError):
        TripletBatch(problem, datas, samples_per_triplet=1, edgel_counts=[None, 0, None])
    with pytest.raises(_abi.HCError):
        TripletBatch(problem, datas, samples_per_triplet=1, edgel_counts=[None, 6000, None])
