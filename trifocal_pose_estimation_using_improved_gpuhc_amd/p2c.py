"""The archived parameter-to-coefficient (P2C) formulation of trifocal_2op1p_30x30.

The archived kernel_GPUHC_trifocal_2op1p_30x30_P2C evaluates dH/dx, dH/dt and H
from index tables whose terms name one *coefficient* k each instead of two
parameters (a, b):

  dHdx_indx_P2C  [row][column][term][part]  parts (c, k, x_u, x_v)        30 x 30 x 8 x 4
  dHdt_indx_P2C  [row][term][part]          parts (c, k, x_u, x_v, x_w)   30 x 16 x 5

and from per-sample coefficient blocks, polynomials in t (coefficient k is the
product p_a(t) * p_b(t) of two linearly interpolated parameters):

  coeffs_hx  [sample][k][order]  coefHx_k(t) = C0 + C1 t + C2 t^2          N x 38 x 3
  coeffs_ht  [sample][k][order]  coefHt_k(t) = D0 + D1 t                   N x 38 x 2

Nothing in the reference computes those blocks; which pair (a, b) coefficient k
stands for follows from the tables alone (derive_coeff_map), and the blocks from
the map (coefficients, the host generator hc_p2c_coefficients).  The library
holds no constant derived from the tables: tables and map are the caller's.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .problem import Problem

NUM_COEFFS = 38                      # Num_of_Coeffs_from_Params + 1 of the archived launcher
HX_SHAPE = (30, 30, 8, 4)
HT_SHAPE = (30, 16, 5)
HX_SIZE, HT_SIZE = 28800, 2400


def _ph_tables(problem: Problem):
    """The PH tables as [row][column][term][part] and [row][term][part]."""
    hx = np.asarray(problem.dHdx_index, np.int64).reshape(30, 8, 5, 30).transpose(3, 0, 1, 2)   # r, c, j, part
    ht = np.asarray(problem.dHdt_index, np.int64).reshape(16, 6, 30).transpose(2, 0, 1)         # r, j, part
    return hx, ht


def _groups(ph_terms, p2c_terms):
    """One entry's terms grouped by (c, sorted x indices): [(pairs, ks)]."""
    g = {}
    for t in ph_terms:
        key = (int(t[0]), tuple(sorted(int(v) for v in t[3:])))
        g.setdefault(key, ([], []))[0].append((min(int(t[1]), int(t[2])), max(int(t[1]), int(t[2]))))
    for t in p2c_terms:
        key = (int(t[0]), tuple(sorted(int(v) for v in t[2:])))
        g.setdefault(key, ([], []))[1].append(int(t[1]))
    return list(g.items())


def derive_coeff_map(problem: Problem, hx_p2c, ht_p2c) -> np.ndarray:
    """(38, 2) int32: coefficient k of the P2C tables is p_a * p_b, a <= b.

    Every entry of the P2C tables holds the terms of the same entry of the PH
    tables in another order, so the terms are matched as multisets on the key
    (c, sorted x indices); a key with several terms leaves its coefficients a
    choice among its pairs, which the other entries narrow.  Raises HCError when
    an entry's terms do not pair up, or a k in 0..37 is missing or not unique."""
    hx_p = np.asarray(hx_p2c, np.int64).reshape(HX_SHAPE)
    ht_p = np.asarray(ht_p2c, np.int64).reshape(HT_SHAPE)
    hx, ht = _ph_tables(problem)
    groups = []
    for r in range(30):
        for c in range(30):
            groups += _groups(hx[r, c], hx_p[r, c])
        groups += _groups(ht[r], ht_p[r])
    cand = {}
    for key, (pairs, ks) in groups:
        if len(pairs) != len(ks):
            raise _abi.HCError(f"P2C tables: the terms with (c, x) = {key} do not pair up with the PH tables'")
        for k in ks:
            cand[k] = cand.get(k, set(pairs)) & set(pairs)
    changed = True
    while changed:   # a resolved coefficient leaves its group's other members one pair fewer
        changed = False
        for _, (pairs, ks) in groups:
            rest = list(pairs)
            open_ks = []
            for k in ks:
                if len(cand[k]) == 1 and next(iter(cand[k])) in rest:
                    rest.remove(next(iter(cand[k])))
                else:
                    open_ks.append(k)
            for k in open_ks:
                narrowed = cand[k] & set(rest)
                if narrowed != cand[k]:
                    cand[k] = narrowed
                    changed = True
    out = np.zeros((NUM_COEFFS, 2), np.int32)
    for k in range(NUM_COEFFS):
        if k not in cand:
            raise _abi.HCError(f"P2C tables: coefficient {k} does not occur")
        if len(cand[k]) != 1:
            raise _abi.HCError(f"P2C tables: coefficient {k} is not unique: {sorted(cand[k])}")
        out[k] = next(iter(cand[k]))
    if set(cand) - set(range(NUM_COEFFS)):
        raise _abi.HCError(f"P2C tables: coefficient indices outside 0..{NUM_COEFFS - 1}")
    return out


def tables_from_ph(problem: Problem):
    """(hx_p2c, ht_p2c, coeff_map) for a caller who has only the PH tables: the
    same terms in the PH tables' order, the distinct parameter pairs numbered in
    sorted order ((33, 33), the constant and the padding coefficient, last)."""
    hx, ht = _ph_tables(problem)
    pairs = set()
    for t in (hx.reshape(-1, 5), ht.reshape(-1, 6)):
        for a, b in t[:, 1:3]:
            pairs.add((min(int(a), int(b)), max(int(a), int(b))))
    pairs = sorted(pairs)
    if len(pairs) != NUM_COEFFS or pairs[-1] != (33, 33):
        raise _abi.HCError(f"{len(pairs)} distinct parameter pairs; the P2C kernel takes {NUM_COEFFS} with (33, 33)")
    index = {p: k for k, p in enumerate(pairs)}
    def conv(t):
        k = np.array([index[(min(int(a), int(b)), max(int(a), int(b)))] for a, b in t[..., 1:3].reshape(-1, 2)],
                     np.int64).reshape(t.shape[:-1])
        return np.ascontiguousarray(np.concatenate([t[..., :1], k[..., None], t[..., 3:]], axis=-1).astype(np.int32))
    return conv(hx).reshape(-1), conv(ht).reshape(-1), np.asarray(pairs, np.int32)


def read_tables(hx_file: str, ht_file: str):
    """The two P2C index files (whitespace-separated integers) as flat int32 arrays."""
    hx = np.loadtxt(hx_file, dtype=np.int64).reshape(-1).astype(np.int32)
    ht = np.loadtxt(ht_file, dtype=np.int64).reshape(-1).astype(np.int32)
    if hx.size != HX_SIZE or ht.size != HT_SIZE:
        raise _abi.HCError(f"P2C tables of {hx.size} and {ht.size} integers (expected {HX_SIZE} and {HT_SIZE})")
    return np.ascontiguousarray(hx), np.ascontiguousarray(ht)


def coefficients(coeff_map, start_params, diff_params):
    """hc_p2c_coefficients: the per-sample blocks (N, 38, 3, 2) and (N, 38, 2, 2)
    float32 of the samples' diff params (N, 34, 2) = target - start."""
    m = np.ascontiguousarray(coeff_map, np.int32).reshape(NUM_COEFFS, 2)
    sp = np.ascontiguousarray(start_params, np.float32).reshape(34, 2)
    dp = np.ascontiguousarray(diff_params, np.float32).reshape(-1, 34, 2)
    n = dp.shape[0]
    chx = np.zeros((n, NUM_COEFFS, 3, 2), np.float32)
    cht = np.zeros((n, NUM_COEFFS, 2, 2), np.float32)
    _abi.call("hc_p2c_coefficients", n, _abi.ptr(m), _abi.ptr(sp), _abi.ptr(dp), _abi.ptr(chx), _abi.ptr(cht))
    return chx, cht


def eval_batched(hx_p2c, ht_p2c, x, coeffs_hx, coeffs_ht, t, device="cuda:0"):
    """hc_trifocal_p2c_eval_batched: dH/dx (n, 30, 30, 2), dH/dt and H (n, 30, 2)
    of the P2C tables at the points x (n, 31, 2), each with its own coefficient
    blocks (n, 38, 3, 2), (n, 38, 2, 2) and its own t (n,)."""
    import torch

    from .tracker import _require_gpu
    dev = _require_gpu(device)
    n = x.shape[0]
    def dev_of(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    hx, ht = dev_of(np.reshape(hx_p2c, -1), np.int32), dev_of(np.reshape(ht_p2c, -1), np.int32)
    if hx.numel() != HX_SIZE or ht.numel() != HT_SIZE:
        raise _abi.HCError(f"P2C tables: {HX_SIZE} and {HT_SIZE} int32 values")
    X, CX, CT, T = dev_of(x, np.float32), dev_of(coeffs_hx, np.float32), dev_of(coeffs_ht, np.float32), \
        dev_of(t, np.float32)
    if tuple(X.shape) != (n, 31, 2) or tuple(CX.shape) != (n, NUM_COEFFS, 3, 2) or \
            tuple(CT.shape) != (n, NUM_COEFFS, 2, 2) or tuple(T.shape) != (n,):
        raise _abi.HCError("P2C evaluation: x (n, 31, 2), blocks (n, 38, 3, 2) and (n, 38, 2, 2), t (n,)")
    HX = torch.empty((n, 30, 30, 2), dtype=torch.float32, device=dev)
    HT = torch.empty((n, 30, 2), dtype=torch.float32, device=dev)
    H = torch.empty((n, 30, 2), dtype=torch.float32, device=dev)
    wsb = int(_abi.lib().hc_trifocal_workspace_size())
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    _abi.call("hc_trifocal_p2c_eval_batched", n, *(_abi.ptr(v) for v in (hx, ht, X, CX, CT, T, HX, HT, H, ws)), wsb,
              _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    _abi.call("hc_trifocal_workspace_status", _abi.ptr(ws))
    return HX.cpu().numpy(), HT.cpu().numpy(), H.cpu().numpy()
