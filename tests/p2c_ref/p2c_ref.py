"""TEST INFRASTRUCTURE ONLY -- ctypes loader of the P2C restatement (p2c_ref.c)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "build", "libp2c_ref.so")
NV, NT, NK = 30, 312, 38

PATH_STATS_DTYPE = np.dtype([("steps", "<i4"), ("corrections", "<i4"), ("inliers21", "<i4"), ("inliers31", "<i4")])


class Settings(C.Structure):
    _fields_ = [("max_steps", C.c_int), ("max_corrections", C.c_int), ("inc_steps", C.c_int),
                ("num_threads", C.c_int)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            subprocess.run(["make", "-s", "-C", HERE], check=True)
        _lib = C.CDLL(LIB_PATH)
        _lib.p2c_one_minus_005.restype = C.c_double
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def one_minus_005() -> float:
    return lib().p2c_one_minus_005()


def coefficients(coeff_map, start_params, diff_params):
    m, sp, dp = _i32(coeff_map), _f32(start_params), _f32(diff_params).reshape(-1, 34, 2)
    n = dp.shape[0]
    chx = np.zeros((n, NK, 3, 2), np.float32)
    cht = np.zeros((n, NK, 2, 2), np.float32)
    lib().p2c_coefficients(C.c_int(n), _p(m), _p(sp), _p(dp), _p(chx), _p(cht))
    return chx, cht


def eval_batched(hx, ht, x, chx, cht, t):
    hx, ht, x, chx, cht, t = _i32(hx), _i32(ht), _f32(x), _f32(chx), _f32(cht), _f32(t)
    n = x.shape[0]
    HX = np.zeros((n, NV, NV, 2), np.float32)
    HT = np.zeros((n, NV, 2), np.float32)
    H = np.zeros((n, NV, 2), np.float32)
    lib().p2c_eval_batched(C.c_int(n), _p(hx), _p(ht), _p(x), _p(chx), _p(cht), _p(t), _p(HX), _p(HT), _p(H))
    return HX, HT, H


def track(start_sols, hx, ht, chx, cht, max_steps=80, max_corrections=3, inc_steps=4, threads=0):
    """(tracks (312N, 31, 2), conv, inf, stats) from the start solutions."""
    hx, ht, chx, cht, ss = _i32(hx), _i32(ht), _f32(chx), _f32(cht), _f32(start_sols)
    n = chx.shape[0]
    tracks = np.ascontiguousarray(np.tile(ss, (n, 1, 1)))
    conv = np.zeros(n * NT, np.uint8)
    inf = np.zeros(n * NT, np.uint8)
    stats = np.zeros(n * NT, PATH_STATS_DTYPE)
    s = Settings(max_steps, max_corrections, inc_steps, threads)
    lib().p2c_track(C.byref(s), C.c_int(n), _p(ss), _p(hx), _p(ht), _p(chx), _p(cht), _p(tracks), _p(conv), _p(inf),
                    _p(stats))
    return tracks, conv, inf, stats
