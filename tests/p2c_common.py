"""What the P2C tests share: the reference's two fixture tables, the map derived
from them, the seed-0 coefficient blocks, the restatement's runs (computed once,
read-only) and FP64 evaluations of both formulations."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "p2c_ref"))

import p2c_ref  # noqa: E402

FIXTURES = os.path.join(HERE, "golden", "p2c")
EPS = 2.0 ** -24


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def fixture_tables():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    return _frozen(*p2c.read_tables(os.path.join(FIXTURES, "dHdx_indx_P2C.txt"),
                                    os.path.join(FIXTURES, "dHdt_indx_P2C.txt")))


@functools.lru_cache(maxsize=None)
def _problem():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_problem
    return load_problem()


@functools.lru_cache(maxsize=None)
def fixture_map():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    return _frozen(p2c.derive_coeff_map(_problem(), *fixture_tables()))


@functools.lru_cache(maxsize=None)
def ph_tables():
    """(hx_p2c, ht_p2c, map) of p2c.tables_from_ph"""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    return _frozen(*p2c.tables_from_ph(_problem()))


@functools.lru_cache(maxsize=None)
def samples(n, dataset=0):
    """(target, diff) of the first n seed-0 samples of a dataset"""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data, prepare_target_params
    tgt, dif, _ = prepare_target_params(_problem(), load_ransac_data(dataset), seed=0, num_samples=n)
    return _frozen(tgt, dif)


@functools.lru_cache(maxsize=None)
def blocks(n, which="fixture"):
    """The restatement generator's coefficient blocks of samples(n) under the fixture map or tables_from_ph's."""
    m = fixture_map() if which == "fixture" else ph_tables()[2]
    return _frozen(*p2c_ref.coefficients(m, _problem().start_params, samples(n)[1]))


@functools.lru_cache(maxsize=None)
def ref_track(n, which="fixture", max_steps=80, max_corrections=3):
    """The restatement's run of samples(n): (tracks, conv, inf, stats), the shape checks.assert_matches_oracle takes."""
    hx, ht = fixture_tables() if which == "fixture" else ph_tables()[:2]
    chx, cht = blocks(n, which)
    return _frozen(*p2c_ref.track(_problem().start_sols, hx, ht, chx, cht, max_steps=max_steps,
                                  max_corrections=max_corrections))


def cplx(a):
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


def perturbed_start_sols(rng, rel=0.01):
    """The 312 start solutions, each entry moved by rel of its size (an exact
    start solution has H ~ 0 and no scale); (312, 31) complex128, x[30] = 1."""
    x = cplx(_problem().start_sols)
    x = x * (1.0 + rel * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)))
    x[:, 30] = 1.0
    return x


def p2c_eval64(hx, ht, x, cHx, cHt, mHx=None):
    """FP64 dH/dx (30, 30), dH/dt, H (30,) of the P2C tables at x (31,) with the
    interpolated coefficients cHx, cHt (38,); also the sums of the terms'
    magnitudes of each output, a coefficient counted as mHx / |cHt| (default |cHx|)."""
    hx = np.asarray(hx).reshape(30, 30, 8, 4)
    ht = np.asarray(ht).reshape(30, 16, 5)
    mHx = np.abs(cHx) if mHx is None else mHx
    xs = x[hx[..., 2]] * x[hx[..., 3]]
    A = (hx[..., 0] * cHx[hx[..., 1]] * xs).sum(-1)
    Am = (np.abs(hx[..., 0]) * mHx[hx[..., 1]] * np.abs(xs)).sum(-1)
    xt = x[ht[..., 2]] * x[ht[..., 3]] * x[ht[..., 4]]
    Ht = -(ht[..., 0] * cHt[ht[..., 1]] * xt).sum(-1)
    H = (ht[..., 0] * cHx[ht[..., 1]] * xt).sum(-1)
    Hm = (np.abs(ht[..., 0]) * mHx[ht[..., 1]] * np.abs(xt)).sum(-1)
    return A, Ht, H, Am, Hm


def ph_eval64(problem, x, p, d):
    """FP64 dH/dx, dH/dt, H of the PH tables at x (31,), p, d (34,)."""
    hx = np.asarray(problem.dHdx_index).reshape(30, 8, 5, 30)    # column, term, part, row
    ht = np.asarray(problem.dHdt_index).reshape(16, 6, 30)       # term, part, row
    A = (hx[:, :, 0] * p[hx[:, :, 1]] * p[hx[:, :, 2]] * x[hx[:, :, 3]] * x[hx[:, :, 4]]).sum(1).T
    xt = x[ht[:, 3]] * x[ht[:, 4]] * x[ht[:, 5]]
    Ht = -(ht[:, 0] * (d[ht[:, 1]] * p[ht[:, 2]] + d[ht[:, 2]] * p[ht[:, 1]]) * xt).sum(0)
    H = (ht[:, 0] * p[ht[:, 1]] * p[ht[:, 2]] * xt).sum(0)
    return A, Ht, H


def coeffs64(coeff_map, s, d):
    """FP64 (C0, C1, C2) of every coefficient from start s and diff d (34,) complex."""
    a, b = np.asarray(coeff_map)[:, 0], np.asarray(coeff_map)[:, 1]
    return s[a] * s[b], s[a] * d[b] + d[a] * s[b], d[a] * d[b]
