"""The drop-in launcher shim (integration/hc_trifocal_shim.cpp).

CPU: the shim compiles against the reference's launcher signatures
(integration/magmaHC-kernels.hpp restating magmaHC-kernels.hpp:24-105, with a
types-only MAGMA stand-in) and exports the four C++-linkage launchers (plus the two archived ..._PH_CodeOpt
ablation launchers) with exactly those parameter lists.

GPU: each of the four launchers, called with the reference's argument lists
(pointer arrays d_startSols_array / d_Track_array as GPU_HC_Solver.cpp:352-353
builds them, bool flags, separate dH/dx / dH/dt tables for the Volta variants),
produces exactly what hc_trifocal_2op1p_30x30_track(_abort) produces.
"""
import ctypes as C
import os
import subprocess

from types import SimpleNamespace

import numpy as np
import pytest

from checks import assert_same_run, assert_untouched, found_ids
from trifocal_pose_estimation_using_improved_gpuhc_amd._abi import ptr as p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "integration", "build", "libhc_shim_test.so")

SIGNATURES = {
    "kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt_TrunPaths":
        "(magma_queue*, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, bool*, bool*, magmaFloatComplex*)",
    "kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt_TrunPaths_Volta":
        "(magma_queue*, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, int*, bool*, bool*, magmaFloatComplex*)",
    "kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt_TrunPaths_TrunRANSAC":
        "(magma_queue*, int, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, float*, float*, bool*, bool*, magmaFloatComplex*, bool*, int*)",
    "kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt_TrunPaths_TrunRANSAC_Volta":
        "(magma_queue*, int, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, int*, float*, float*, bool*, bool*, magmaFloatComplex*, "
        "bool*, int*)",
    # archived ablation launchers (arxived_GPU_code/gpu-kernels/magmaHC-kernels.hpp:61-96)
    "kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt":
        "(magma_queue*, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, bool*, bool*, magmaFloatComplex*)",
    "kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt_Volta":
        "(magma_queue*, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, int*, bool*, bool*, magmaFloatComplex*)",
    "kernel_GPUHC_trifocal_2op1p_30x30_PH":
        "(magma_queue*, int, int, int, int, magmaFloatComplex**, magmaFloatComplex**, magmaFloatComplex*, "
        "magmaFloatComplex*, magmaFloatComplex*, int*, int*, bool*, bool*, magmaFloatComplex*)",
}


def test_shim_exports_reference_signatures():
    assert os.path.exists(SHIM), "integration shim not built (__graft_entry__.build())"
    out = subprocess.run(["nm", "-DC", SHIM], capture_output=True, text=True, check=True).stdout
    exported = {line.split(" T ", 1)[1].strip() for line in out.splitlines() if " T " in line}
    for name, sig in SIGNATURES.items():
        assert name + sig in exported, f"{name}{sig} not exported"


def test_shim_exports_reserve_and_status():
    """The two calls GPU_HC_Solver adds (integration/hc_trifocal_shim.h): C linkage."""
    assert os.path.exists(SHIM), "integration shim not built (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", SHIM], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("hc_trifocal_shim_reserve", "hc_trifocal_shim_status", "hc_trifocal_shim_info"):
        assert name in exported, name


def _lib():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    _abi.lib()                      # the shim binds to the already loaded libhc_trifocal.so
    L = C.CDLL(SHIM)
    L.shim_queue_create.restype = C.c_void_p
    L.shim_queue_create.argtypes = [C.c_void_p]
    L.shim_queue_destroy.argtypes = [C.c_void_p]
    L.hc_trifocal_shim_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.hc_trifocal_shim_status.argtypes = [C.c_void_p]
    L.hc_trifocal_shim_info.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    for f in ("shim_trunpaths", "shim_trunpaths_volta", "shim_trunransac", "shim_trunransac_volta",
              "shim_ph_codeopt", "shim_ph_codeopt_volta", "shim_ph"):
        getattr(L, f).restype = C.c_double
    return L


def _reference_layout(problem, tracker, tgt, dif):
    """The reference's device layout (GPU_HC_Solver.cpp:137-184,335-362): start
    sols and tracks as 31-complex columns, addressed through per-track pointer
    arrays (d_startSols_array / d_Track_array), the parameters of tgt's
    samples and the index tables, unified and separate.  outputs(n): tracks at
    the start solutions, their pointer array and cleared flags for a launch of
    n samples; common(o): the launchers' shared argument run."""
    import torch
    dev, s = tracker.device, tracker.settings
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ss = up(problem.start_sols)
    lay = SimpleNamespace(ss=ss, sp=up(problem.start_params), tp=up(tgt), dp=up(dif), U=up(problem.unified_index),
                          hx=up(problem.dHdx_index.reshape(-1)), ht=up(problem.dHdt_index.reshape(-1)),
                          ssa=torch.tensor([ss.data_ptr() + k * 31 * 8 for k in range(312)], dtype=torch.int64,
                                           device=dev))

    def outputs(n):
        o = SimpleNamespace(tracks=ss.unsqueeze(0).expand(n, -1, -1, -1).reshape(n * 312, 31, 2).contiguous(),
                            conv=torch.zeros(312 * n, dtype=torch.bool, device=dev),
                            inf=torch.zeros(312 * n, dtype=torch.bool, device=dev))
        o.tra = torch.tensor([o.tracks.data_ptr() + b * 31 * 8 for b in range(312 * n)], dtype=torch.int64, device=dev)
        o.host = lambda: dict(tracks=o.tracks.cpu().numpy(), converge=o.conv.cpu().numpy().astype(np.uint8),
                              infinity=o.inf.cpu().numpy().astype(np.uint8))
        return o

    lay.outputs = outputs
    lay.common = lambda o: [C.c_int(s.max_steps), C.c_int(s.max_corrections), C.c_int(s.delta_t_inc_steps),
                            p(lay.ssa), p(o.tra), p(lay.sp), p(lay.tp), p(lay.dp)]
    return lay


def _assert_same_flags_and_tracks(got, ref, where=None):
    """The launchers report no step or correction counts."""
    assert_same_run(got, ref["tracks"], ref["converge"], ref["infinity"], None, None, where)


@pytest.mark.gpu
@pytest.mark.parametrize("abort,truncate,volta,N", [
    (a, t, v, 3) for (a, t) in [(False, True), (True, True), (False, False)] for v in (False, True)] + [
    (False, True, False, 100)])   # enough paths for time slicing: suspended x goes through the pointer arrays
def test_shim_launchers_match_abi(problem, samples100, tracker, ransac0, abort, truncate, volta, N):
    """truncate=False: the archived ..._PH_CodeOpt[_Volta] launchers against
    hc_trifocal_2op1p_30x30_track_ph_codeopt."""
    import torch
    L = _lib()
    dev = tracker.device
    tgt, dif, _ = samples100
    ref = tracker.track(tgt[:N], dif[:N], abort=abort, truncate=truncate).host()
    lay = _reference_layout(problem, tracker, tgt[:N], dif[:N])
    o = lay.outputs(N)
    found = torch.zeros(1, dtype=torch.bool, device=dev)
    bidx = torch.full((312 * N,), -1, dtype=torch.int32, device=dev)
    q = L.shim_queue_create(p(torch.cuda.current_stream(dev)))
    tables = [p(lay.hx), p(lay.ht)] if volta else [p(lay.U)]
    if abort:
        E = tracker.edgels
        fn = L.shim_trunransac_volta if volta else L.shim_trunransac
        rv = fn(C.c_void_p(q), C.c_int(N), C.c_int(E.shape[0]), *lay.common(o), *tables, p(E), p(tracker.K), p(o.conv),
                p(o.inf), p(found), p(bidx))
    elif truncate:
        fn = L.shim_trunpaths_volta if volta else L.shim_trunpaths
        rv = fn(C.c_void_p(q), C.c_int(N), *lay.common(o), *tables, p(o.conv), p(o.inf))
    else:
        fn = L.shim_ph_codeopt_volta if volta else L.shim_ph_codeopt
        rv = fn(C.c_void_p(q), C.c_int(N), *lay.common(o), *tables, p(o.conv), p(o.inf))
    torch.cuda.synchronize(dev)
    L.shim_queue_destroy(C.c_void_p(q))
    assert rv == 0.0
    got = o.host()
    if not abort:
        _assert_same_flags_and_tracks(got, ref)
    else:
        # which paths get skipped depends on scheduling; every path the shim tracked
        # equals the abort-off result and found ids are the direct ABI's passing set
        full = tracker.track(tgt[:N], dif[:N]).host()
        assert bool(found.item())
        ids = found_ids(dict(batch_index=bidx.cpu().numpy()))
        assert len(ids) and (full["converge"][ids] == 1).all()
        # the launchers report no step counts: a path that left its start solution was tracked
        start = np.tile(problem.start_sols[None, :, :30], (N, 1, 1, 1)).reshape(-1, 30, 2)
        moved = ~np.all(got["tracks"][:, :30] == start, axis=(1, 2))
        _assert_same_flags_and_tracks(got, full, where=moved)
        assert_untouched(got, problem.start_sols, ~moved, allow_empty=True)


@pytest.mark.gpu
def test_shim_ph_launcher_matches_abi(problem, samples100, tracker):
    """The archived ..._PH launcher (separate dH/dx, dH/dt tables) against
    hc_trifocal_2op1p_30x30_track_ph."""
    import torch
    L = _lib()
    dev = tracker.device
    N = 2
    tgt, dif, _ = samples100
    ref = tracker.track(tgt[:N], dif[:N], truncate=False, explicit_rk=True).host()
    lay = _reference_layout(problem, tracker, tgt[:N], dif[:N])
    o = lay.outputs(N)
    q = L.shim_queue_create(p(torch.cuda.current_stream(dev)))
    rv = L.shim_ph(C.c_void_p(q), C.c_int(N), *lay.common(o), p(lay.hx), p(lay.ht), p(o.conv), p(o.inf))
    torch.cuda.synchronize(dev)
    L.shim_queue_destroy(C.c_void_p(q))
    assert rv == 0.0
    _assert_same_flags_and_tracks(o.host(), ref)


@pytest.mark.gpu
def test_shim_reserved_stream_never_allocates(problem, samples100, tracker):
    """hc_trifocal_shim_reserve (called from GPU_HC_Solver::Allocate_Arrays)
    sizes the stream's workspace for time slicing up front: launches of up to
    that many samples (plain and Volta) then never allocate on the launch path,
    hc_trifocal_shim_status reports success after the launch, and the results
    equal the ABI's.  A launch on a stream that was not reserved still works
    (the lazy fallback) and is counted."""
    import torch
    L = _lib()
    dev = tracker.device
    N = 100
    tgt, dif, _ = samples100
    ref = tracker.track(tgt[:N], dif[:N]).host()
    stream = torch.cuda.Stream(dev)
    q = L.shim_queue_create(p(stream))
    s = tracker.settings
    assert L.hc_trifocal_shim_reserve(C.c_void_p(q), N, s.max_steps) == 0
    wsb, grows = C.c_size_t(0), C.c_int(-1)
    assert L.hc_trifocal_shim_info(C.c_void_p(q), C.byref(wsb), C.byref(grows)) == 0
    reserved = wsb.value
    assert reserved == int(tracker.L.hc_trifocal_workspace_size_for_steps(N, s.max_steps)) and grows.value == 0
    lay = _reference_layout(problem, tracker, tgt[:N], dif[:N])
    torch.cuda.synchronize(dev)
    for volta, n in ((False, N), (True, N), (False, 7)):
        o = lay.outputs(n)
        torch.cuda.synchronize(dev)
        if volta:
            L.shim_trunpaths_volta(C.c_void_p(q), C.c_int(n), *lay.common(o), p(lay.hx), p(lay.ht), p(o.conv), p(o.inf))
        else:
            L.shim_trunpaths(C.c_void_p(q), C.c_int(n), *lay.common(o), p(lay.U), p(o.conv), p(o.inf))
        assert L.hc_trifocal_shim_status(C.c_void_p(q)) == 0
        _assert_same_flags_and_tracks(o.host(), {k: ref[k][:312 * n] for k in ("tracks", "converge", "infinity")})
    assert L.hc_trifocal_shim_info(C.c_void_p(q), C.byref(wsb), C.byref(grows)) == 0
    assert grows.value == 0 and wsb.value == reserved
    L.shim_queue_destroy(C.c_void_p(q))
