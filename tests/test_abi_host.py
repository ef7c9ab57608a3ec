"""CPU tests of the C-ABI boundary and the native host data layer.

* the library exports exactly the entry points include/*.h declare;
* the binding's signature table agrees with the prototypes, and its struct
  mirrors with the layouts the C compiler gives the headers;
* argument validation returns the documented hcStatus codes without touching
  a device (no compute call is made here);
* the host layer (readers, RANSAC sample generation, sample split, solution
  counting -- include/hc_host.h) agrees bit for bit with the oracle's
  independent C restatement of Data_Reader.cpp / GPU_HC_Solver.cpp:252-306 /
  Evaluations.cpp:145-182.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def _prototypes(header):
    """{name: (return type, [parameter, ...])} of the functions a C header
    declares (outside comments); `(void)` is no parameter."""
    src = open(os.path.join(INCLUDE, header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def _declared_c_functions(header):
    """Function names declared in a C header (outside comments)."""
    return set(_prototypes(header))


def _headers():
    return [h for h in sorted(os.listdir(INCLUDE)) if h.endswith(".h")]


def _all_declared():
    """Every function the public headers declare (include/*.h)."""
    names = set()
    for h in _headers():
        names |= _declared_c_functions(h)
    return names


# C scalar type of a prototype -> the ctypes class the signature table must give it
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "double": C.c_double,
            "uint64_t": C.c_uint64}
_RETURNS = {"void": None, "hcStatus": C.c_int, "int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t,
            "const char *": C.c_char_p}


def _is_pointer_class(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_signature_table_matches_the_prototypes():
    """Every entry of _abi.SIGNATURES against its prototype in include/*.h: the
    same set of names, the parameter count, pointer (`*` or hcStream) against
    scalar for each parameter -- a scalar also by its type --, and the return
    type's class."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    protos = {}
    for h in _headers():
        for name, p in _prototypes(h).items():
            assert protos.setdefault(name, p) == p, f"{name} is declared twice, differently"
    assert len(protos) == 50
    assert {s.name for s in _abi.SIGNATURES} == set(protos)
    assert len(_abi.SIGNATURES) == len(protos), "a name is listed twice"
    for s in _abi.SIGNATURES:
        ret, params = protos[s.name]
        assert ret in _RETURNS, f"{s.name}: return type {ret!r}"
        assert s.restype is _RETURNS[ret], f"{s.name}: returns {ret!r}, bound as {s.restype}"
        assert len(s.argtypes) == len(params), f"{s.name}: {len(params)} parameters, {len(s.argtypes)} argtypes"
        for k, (p, t) in enumerate(zip(params, s.argtypes)):
            if "*" in p or p.startswith("hcStream "):
                assert _is_pointer_class(t), f"{s.name} parameter {k} ({p}) is a pointer, bound as {t}"
            else:
                ctype = " ".join(w for w in p.split()[:-1] if w != "const")
                assert ctype in _SCALARS, f"{s.name} parameter {k}: type {ctype!r}"
                assert t is _SCALARS[ctype], f"{s.name} parameter {k} ({p}) is bound as {t}"
    # what lib() bound is the table
    L = _abi.lib()
    for s in _abi.SIGNATURES:
        fn = getattr(L, s.name)
        assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes), s.name


def _c_compiler():
    import shutil
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no C compiler found"
    return cc


def test_struct_mirrors_match_the_headers_by_the_c_compiler(tmp_path):
    """sizeof and every field's offsetof of the mirrored structs, from the
    headers through the host C compiler, equal the ctypes classes' and the two
    numpy dtypes' (tracker.PATH_STATS_DTYPE, multi.GROUP_DTYPE)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, multi, tracker
    structs = [_abi.hcTrackSettings, _abi.hcTrackArgs, _abi.hcAbortArgs, _abi.hcTripletGroup,
               _abi.hcGroupedAbortArgs, _abi.hcJointGate, _abi.hcIpcHandle, _abi.hcPoseSelection,
               _abi.hcTrifocalSelection]
    # [(C struct, field names, size, field offsets)] as Python has them
    mirrors = [(s.__name__, [f[0] for f in s._fields_], C.sizeof(s), [getattr(s, f[0]).offset for f in s._fields_])
               for s in structs]
    mirrors += [(name, list(dt.names), dt.itemsize, [dt.fields[f][1] for f in dt.names])
                for name, dt in (("hcPathStats", tracker.PATH_STATS_DTYPE), ("hcTripletGroup", multi.GROUP_DTYPE))]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "hc_trifocal.h"', '#include "hc_pose.h"',
             'int main(void) {']
    for name, fields, _, _ in mirrors:
        args = "".join(f", offsetof({name}, {f})" for f in fields)
        lines.append(f'    printf("{"%zu " * (1 + len(fields))}\\n", sizeof({name}){args});')
    lines += ['    return 0;', '}', '']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([_c_compiler(), "-I", INCLUDE, "-o", str(exe), str(src)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    assert len(out) == len(mirrors) == 11
    for (name, fields, size, offsets), line in zip(mirrors, out):
        got = [int(v) for v in line.split()]
        assert got[0] == size, f"sizeof({name}): C {got[0]}, Python {size}"
        assert got[1:] == offsets, f"{name}: C offsets {dict(zip(fields, got[1:]))}, Python {offsets}"
    # the nine structs' sizes at ABI version 2
    assert [m[2] for m in mirrors[:9]] == [12, 104, 56, 24, 56, 16, 64, 136, 136]


def test_headers_declare_the_bound_symbols():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    declared = _all_declared()
    assert declared == set(_abi.DECLARED_SYMBOLS)


def test_library_exports_every_declared_symbol():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    declared = _all_declared()
    missing = declared - exported
    assert not missing, f"declared but not exported: {sorted(missing)}"
    L = _abi.lib()
    for name in declared:
        assert getattr(L, name) is not None


def test_workspace_size_and_version():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    ws = int(L.hc_trifocal_workspace_size())
    assert 64 <= ws < (1 << 20)
    assert ws % 256 == 0
    assert b"gfx950" in L.hc_trifocal_version()


def test_abi_version_and_build_id():
    """The binding refuses a library of another struct layout; the build id
    names the library's device code (bench.py selects its profiles by it)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    assert L.hc_trifocal_abi_version() == _abi.ABI_VERSION == 2
    hdr = open(os.path.join(ROOT, "include", "hc_trifocal.h")).read()
    assert "#define HC_TRIFOCAL_ABI_VERSION 2" in hdr
    bid = _abi.build_id()
    assert bid.startswith("v") and "+" in bid and len(bid.split("+")[1]) == 12
    assert bid == _abi.build_id(_abi.PRODUCT_LIB_PATH)


def test_workspace_size_for_time_slicing():
    """hc_trifocal_workspace_size_for(N): the base workspace + the time-slicing
    area: ring counters (1 KB), a 256-B suspend block per path and an 8-B ring
    entry per possible suspension -- at most (max_steps + 1) / 3 per path,
    never reused within a launch (+1 per path, + 4096 spare entries for the
    re-pushes of abandoned tickets).  The plain form assumes max_steps = 80."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    base = int(L.hc_trifocal_workspace_size())
    s0, s1, s100 = (int(L.hc_trifocal_workspace_size_for(n)) for n in (0, 1, 100))
    assert base < s0 <= s1 < s100
    assert s100 % 256 == 0
    per_path = 256 + 8 * (81 // 3 + 1)
    assert per_path * 312 * 100 + 8 * 4096 <= s100 - base <= per_path * 312 * 100 + 8 * 4096 + 2048
    assert int(L.hc_trifocal_workspace_size_for(-5)) == s0
    assert int(L.hc_trifocal_workspace_size_for_steps(100, 80)) == s100
    s200 = int(L.hc_trifocal_workspace_size_for_steps(100, 200))
    assert s200 - s100 >= 8 * 312 * 100 * (201 // 3 - 81 // 3)


def test_invalid_arguments_are_rejected_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    ws = int(L.hc_trifocal_workspace_size())
    dummy = C.c_void_p(0x1000)          # never dereferenced: validation fails first
    a = _abi.hcTrackArgs()
    a.sub_ransac_iters = 1
    a.settings = _abi.hcTrackSettings(80, 3, 4)
    # null args / null workspace
    assert L.hc_trifocal_2op1p_30x30_track(None, dummy, ws, None) == 1
    assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), None, ws, None) == 2
    assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), dummy, ws - 1, None) == 2
    # required device pointers missing
    assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), dummy, ws, None) == 1
    # negative sizes / settings
    a.sub_ransac_iters = -1
    assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), dummy, ws, None) == 1
    a.sub_ransac_iters = 1
    for f in ("start_sols", "tracks", "start_params", "target_params", "diff_params", "unified_index",
              "converge", "infinity"):
        setattr(a, f, 0x1000)
    for bad in ((-1, 3, 4), (80, -1, 4), (80, 3, -1)):
        a.settings = _abi.hcTrackSettings(*bad)
        assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), dummy, ws, None) == 1, bad
    a.settings = _abi.hcTrackSettings(80, 3, 4)
    # too many paths for the int32 batch index of the reference interface
    a.sub_ransac_iters = (1 << 31) // 312 + 1
    assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), dummy, ws, None) == 1
    # abort mode needs its RANSAC arrays
    a.sub_ransac_iters = 1
    ab = _abi.hcAbortArgs()
    assert L.hc_trifocal_2op1p_30x30_track_abort(C.byref(a), None, dummy, ws, None) == 1
    assert L.hc_trifocal_2op1p_30x30_track_abort(C.byref(a), C.byref(ab), dummy, ws, None) == 1
    # zero samples is a no-op success (reference: empty grid)
    a.sub_ransac_iters = 0
    assert L.hc_trifocal_2op1p_30x30_track(C.byref(a), dummy, ws, None) == 0
    # component entry points
    assert L.hc_cgesv_30x30_batched(-1, None, None, None, None) == 1
    assert L.hc_cgesv_30x30_batched(4, None, None, None, None) == 1
    assert L.hc_cgesv_30x30_batched(0, None, None, None, None) == 0
    assert L.hc_trifocal_eval_batched(4, None, None, None, None, None, None, None, dummy, ws, None) == 1
    u = C.c_void_p(0x2000)
    assert L.hc_trifocal_eval_batched(0, u, None, None, None, None, None, None, None, 0, None) == 2
    d = C.c_double(0)
    assert L.hc_trifocal_read_timings(None, C.byref(d)) == 1


def test_host_readers_match_oracle(problem, oracle):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.problem import problem_dir
    ss, sp, dhdx, dhdt = oracle.read_problem(problem_dir())
    assert np.array_equal(problem.start_sols.view(np.uint32), ss.view(np.uint32))
    assert np.array_equal(problem.start_params.view(np.uint32), sp.view(np.uint32))
    assert np.array_equal(problem.dHdx_index, dhdx)
    assert np.array_equal(problem.dHdt_index, dhdt)
    assert np.all(problem.start_sols[:, 30] == np.array([1.0, 0.0], np.float32))
    assert np.all(problem.start_params[33] == np.array([1.0, 0.0], np.float32))


@pytest.mark.parametrize("index", [0, 1, 2])
def test_edgel_reader_matches_oracle(oracle, index):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data
    from trifocal_pose_estimation_using_improved_gpuhc_amd.problem import ransac_dir
    d = load_ransac_data(index)
    loc, tan = oracle.read_edgels(os.path.join(ransac_dir(), "Triplet_Edgels", f"Triplet_Edgels_{index:03d}.txt"))
    assert np.array_equal(d.locations.view(np.uint32), loc.view(np.uint32))
    assert np.array_equal(d.tangents.view(np.uint32), tan.view(np.uint32))
    K = oracle.read_floats(os.path.join(ransac_dir(), "Intrinsic_Matrix.txt"), 9)
    assert np.array_equal(d.K, K)
    # GT poses: R row-major (orthonormal) then t
    for P in (d.pose21, d.pose31):
        R = P[:9].reshape(3, 3).astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5


@pytest.mark.parametrize("n,g", [(100, 1), (8000, 8), (1001, 8), (7, 8), (1000, 3)])
def test_split_samples_rule(n, g):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import split_samples
    sub = split_samples(n, g)
    ref = np.array([n // g + (1 if k < n % g else 0) for k in range(g)])   # GPU_HC_Solver.cpp:85-88
    assert np.array_equal(sub, ref)
    assert sub.sum() == n


@pytest.mark.parametrize("n,g,seed", [(100, 1, 0), (37, 4, 0), (64, 8, 7)])
def test_prepare_target_params_matches_oracle(problem, ransac0, oracle, n, g, seed):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import prepare_target_params, split_samples
    tgt, dif, picked = prepare_target_params(problem, ransac0, seed=seed, num_samples=n, num_gpus=g)
    t2, d2, p2 = oracle.prepare_target_params(seed, split_samples(n, g), ransac0.locations, ransac0.tangents,
                                              problem.start_params)
    assert np.array_equal(picked, p2)
    assert np.array_equal(tgt.view(np.uint32), t2.view(np.uint32))
    assert np.array_equal(dif.view(np.uint32), d2.view(np.uint32))
    # reference draw rule: i0 != i1 and i1 != i2 (i0 == i2 allowed), indices in range
    assert np.all(picked[:, 0] != picked[:, 1]) and np.all(picked[:, 1] != picked[:, 2])
    assert picked.min() >= 0 and picked.max() < ransac0.locations.shape[0]
    # params 30..33 are the constants of GPU_HC_Solver.cpp:290-296
    assert np.array_equal(tgt[:, 30:34, 0], np.tile([1.0, 0.5, 1.0, 1.0], (n, 1)).astype(np.float32))


def test_sample_k_is_independent_of_gpu_count(problem, ransac0):
    """gpu-major order: sharding over G GPUs reproduces the same sample sequence."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import prepare_target_params
    t1, _, p1 = prepare_target_params(problem, ransac0, seed=0, num_samples=64, num_gpus=1)
    t8, _, p8 = prepare_target_params(problem, ransac0, seed=0, num_samples=64, num_gpus=8)
    assert np.array_equal(p1, p8) and np.array_equal(t1, t8)


def test_count_solutions_matches_oracle(oracle):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import count_solutions
    rng = np.random.default_rng(5)
    n = 3
    tracks = rng.standard_normal((312 * n, 31, 2)).astype(np.float32)
    tracks[::3, :30, 1] = 0.0               # a third are real
    tracks[1::7, 4, 1] = 5e-5               # within the 1e-4 imaginary tolerance
    conv = (rng.random(312 * n) < 0.4).astype(np.uint8)
    inf = ((rng.random(312 * n) < 0.2) & (conv == 0)).astype(np.uint8)
    assert count_solutions(tracks, conv, inf) == tuple(oracle.count_solutions(tracks, conv, inf))
    assert count_solutions(tracks, np.zeros_like(conv), np.zeros_like(inf)) == (0, 0, 0)


def test_write_converged_sols_layout(tmp_path):
    """hc_write_converged_sols == Evaluations::Write_Converged_Sols byte layout
    (Evaluations.cpp:120-143): header per sample, global batch id, 30 re/im lines
    printed with std::setprecision(20) (== printf %.20g of the float)."""
    import ctypes as C

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    rng = np.random.default_rng(3)
    N = 2
    tr = rng.standard_normal((312 * N, 31, 2)).astype(np.float32)
    tr[5, 3, 0] = 0.0
    tr[7, 4, 1] = -0.0
    tr[9, 1, 0] = 1e-30
    conv = (rng.random(312 * N) < 0.1).astype(np.uint8)
    f = str(tmp_path / "sols.txt")
    n = _abi.lib().hc_write_converged_sols(f.encode(), C.c_int(N), C.c_void_p(tr.ctypes.data),
                                           C.c_void_p(conv.ctypes.data))
    assert n == int(conv.sum())
    exp = []
    for ri in range(N):
        exp.append(f"-------------------- RANSAC Iteration {ri + 1} --------------------\n\n")
        for bs in range(312):
            b = ri * 312 + bs
            if conv[b]:
                exp.append(f"{b}\n")
                for v in range(30):
                    exp.append(f"{float(tr[b, v, 0]):.20g}\t{float(tr[b, v, 1]):.20g}\n")
                exp.append("\n")
        exp.append("\n")
    assert open(f).read() == "".join(exp)
