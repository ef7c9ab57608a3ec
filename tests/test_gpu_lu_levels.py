"""GPU tests of the tracker LU's fused levels (hc_lu.hpp lu_level): the
throughput tracker's solve alone (hc_cgesv_30x30_struct_batched) against the
oracle's LU, system by system, on inputs that reach every exit of a fused
level, and the throughput kernel against the oracle's tracker.

Bar: identical values (conftest.same: NaN == NaN, +0 == -0)."""
import numpy as np
import pytest

from checks import SMALL_NEVER, assert_matches_oracle, launch_mode
from conftest import same

pytestmark = pytest.mark.gpu

NV = 30
FUSED = range(18)


@pytest.fixture(scope="module")
def structure():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    pat = [int(L.hc_lu_struct_pattern(r)) for r in range(NV)]
    cand = [[r for r in range(NV) if (int(L.hc_lu_candidates(i)) >> r) & 1] for i in range(NV)]
    mask = np.array([[(pat[r] >> c) & 1 for c in range(NV)] for r in range(NV)], bool)
    return pat, cand, mask


def _random_on_pattern(rng, mask, n):
    A = rng.standard_normal((n, NV, NV, 2)).astype(np.float32)
    A *= mask[None, :, :, None]
    return A


def _isolate(A, pat, cand, rows, step):
    """Rows `rows` reach pivot step `step` with their input entries: their
    entries in the earlier pivot columns that could touch them are zero, so
    they take a zero multiple of every earlier pivot row."""
    for r in rows:
        for i in range(step):
            if r in cand[i]:
                A[r, i, :] = 0.0


def _tie_pairs(pat, cand, step):
    """Pairs of candidate rows that hold column `step` structurally: one inside
    a lane triple and, for a 6-row chain, one across its two triples."""
    rows = [r for r in cand[step] if (pat[r] >> step) & 1]
    inside = [(a, b) for a in rows for b in rows if a < b and a // 3 == b // 3][:1]
    across = [(a, b) for a in rows for b in rows if a < b and a // 3 != b // 3][:1]
    return inside + across


# The 6-row chains whose later pivot columns reach one of their triples only by
# fill-in.  X: triples lo and hi share the earlier pivot column c0; lo holds
# column ca, hi holds cb.  Y: lo and hi have pivot columns c1 and c2 of their
# own, share cj, and lo's first two rows hold ca, hi's first two cb.
FAMILY_X = [((3, 4, 5), (12, 13, 14), 0, 3, 6), ((6, 7, 8), (15, 16, 17), 1, 4, 7)]
FAMILY_Y = [((18, 19, 20), (24, 25, 26), 8, 9, 12, 13, 14), ((21, 22, 23), (27, 28, 29), 10, 11, 15, 16, 17)]
BIG, HALF, PIV, TIE = (16.0, 0.0), (8.0, 0.0), (4.0, 12.0), (8.0, 0.0)   # -(8/16) * (4 + 12i): |re| + |im| = 8


def _cross_tie(A, step):
    """Sets entries of A (random on the pattern) so that at pivot step `step`
    one row of each triple of the chain ties for the maximum, the row of the
    triple that lacks the column structurally through fill-in: it takes
    -(8 / 16) * (4 + 12i) from an earlier pivot row, exactly, and the other
    row holds 8.  Returns the two rows, or None for a step without such a chain."""
    for lo, hi, c0, ca, cb in FAMILY_X:
        (a0, a1, a2), (b0, b1, b2) = lo, hi
        if step == ca:
            A[a0, c0], A[a0, ca], A[b0, c0] = BIG, PIV, HALF
            A[a1, c0] = A[a2, c0] = A[b1, c0] = A[b2, c0] = 0.0
            A[a1, ca] = TIE
            A[a2, ca] *= 0.25
            return a1, b0
        if step == cb:
            A[b0, c0], A[b0, cb], A[a0, c0] = BIG, PIV, HALF
            A[a1, c0] = A[a2, c0] = A[b1, c0] = A[b2, c0] = 0.0
            A[a2, ca] = BIG              # step ca's pivot row: no column cb
            A[a0, ca] *= 0.25
            A[a1, ca] *= 0.25
            A[b1, cb] = TIE
            A[b2, cb] *= 0.25
            return a0, b1
    for lo, hi, c1, c2, cj, ca, cb in FAMILY_Y:
        (a0, a1, a2), (b0, b1, b2) = lo, hi
        if step == ca:
            A[a0, c1] = A[a1, c1] = A[b0, c2] = 0.0
            A[a0, cj], A[a0, ca], A[b0, cj] = BIG, PIV, HALF
            A[a1, cj] = 0.0
            A[a1, ca] = TIE
            A[b1, cj] *= 0.25
            A[b2, cj] *= 0.25
            A[a2, cj] *= 0.25
            return a1, b0
        if step == cb:
            A[b0, c2] = A[b1, c2] = A[a0, c1] = A[a1, c1] = 0.0
            A[b0, cj], A[b0, cb], A[a0, cj] = BIG, PIV, HALF
            A[b1, cj] = A[a1, cj] = 0.0
            A[a0, ca] = 0.0
            A[a1, ca] = BIG              # step ca's pivot row: no column cb
            A[b1, cb] = TIE
            A[a2, cj] *= 0.25
            A[b2, cj] *= 0.25
            return a0, b1
    return None


def _keys_at(A, step):
    """|re| + |im| of column `step` in the rows not pivoted yet when partial-pivot
    elimination reaches that step (complex64; the constructed entries are exact
    in any rounding), as {row: key}."""
    M = (A[..., 0] + 1j * A[..., 1]).astype(np.complex64)
    free = list(range(NV))
    cabs1 = lambda z: np.float32(abs(np.float32(z.real)) + abs(np.float32(z.imag)))
    for i in range(step):
        p = max(free, key=lambda r: (cabs1(M[r, i]), -r))
        free.remove(p)
        if cabs1(M[p, i]) == 0:
            continue
        for r in free:
            l = np.complex64(M[r, i] / M[p, i])
            if l != 0:
                M[r, i + 1:] = (M[r, i + 1:] - l * M[p, i + 1:]).astype(np.complex64)
    return {r: cabs1(M[r, step]) for r in free}


@pytest.fixture(scope="module")
def batch(problem, oracle, samples100, structure):
    """The mixed batch (every case, fallback and common path in the same
    waves) and the oracle's solutions, computed once."""
    pat, cand, mask = structure
    rng = np.random.default_rng(2024)
    tgt, dif, _ = samples100
    As, bs, what = [], [], []

    def add(A, b, name):
        As.append(A.astype(np.float32)); bs.append(b.astype(np.float32)); what.append(name)

    def plain():
        return _random_on_pattern(rng, mask, 1)[0], rng.standard_normal((NV, 2))

    # tracker Jacobians and right-hand sides at N = 2 samples (start solutions pushed along t)
    for k in range(6):
        x = problem.start_sols[int(rng.integers(0, 312))].copy()
        x[:30] += (rng.standard_normal((30, 2)) * 10 ** rng.uniform(-4, -1)).astype(np.float32)
        s = int(rng.integers(0, 2))
        p = oracle.param_homotopy(float(np.float32(rng.uniform(0, 1))), problem.start_params, tgt[s])
        add(oracle.eval_hx(problem.dHdx_index, x, p), oracle.eval_ht(problem.dHdt_index, x, p, dif[s]), "jacobian")
    # random values on the structure, a different matrix in each half
    for k in range(2):
        add(*plain(), "random")
    # an exact tie of |re| + |im| at every fused step: the first four beside an
    # untied half, the others in both halves of a wave at different steps
    ties = 0
    for step in FUSED:
        for (ra, rb) in _tie_pairs(pat, cand, step):
            A, b = plain()
            _isolate(A, pat, cand, (ra, rb), step)
            A[ra, step] = (8.0, 0.0)
            A[rb, step] = (3.0, 5.0)
            add(A, b, f"tie {step} {ra} {rb}")
            ties += 1
            if ties <= 4:
                add(*plain(), "random beside a tie")
    # ... and for the steps whose column reaches one triple of the chain only by
    # fill-in, a tie between the two triples built through that fill-in
    for step in FUSED:
        A, b = plain()
        rows = _cross_tie(A, step)
        if rows is None:
            continue
        keys = _keys_at(A, step)
        assert keys[rows[0]] == keys[rows[1]] == max(keys.values()) == 8.0, (step, rows, keys)
        assert rows[0] // 3 != rows[1] // 3 and all(r in cand[step] for r in rows)
        add(A, b, f"tie {step} {rows[0]} {rows[1]}")
    # both halves tied at different steps
    for step in (0, 2):
        ra, rb = _tie_pairs(pat, cand, step)[0]
        A, b = plain()
        A[ra, step] = (-4.0, 4.0)
        A[rb, step] = (0.0, -8.0)
        add(A, b, f"tie {step}")
    for step in (2, 5, 9):     # an all-zero candidate column
        A, b = plain()
        A[:, step] = 0.0
        add(A, b, f"zero column {step}")
    for step in (1, 8):        # a pivot below 2^-90
        A, b = plain()
        A[:, step] *= np.float32(2.0 ** -100)
        add(A, b, f"tiny pivot {step}")
    A, b = plain(); A[3, 3, 0] = np.nan; add(A, b, "NaN at position 3")
    A, b = plain(); A[4, 3, 1] = np.nan; add(A, b, "NaN elsewhere in column 3")
    A, b = plain(); A[2, 2, 0] = np.nan; add(A, b, "NaN at position 2")
    A, b = plain(); A[5, 3, 0] = np.inf; add(A, b, "inf")
    A, b = plain(); A[20, 8, 0] = np.float32(2.0 ** 70); add(A, b, "entry above 2^64")
    while len(As) < 64:
        add(*plain(), "random")
    As, bs = np.stack(As)[:64], np.stack(bs)[:64]
    for A in As:
        assert not (A[~mask] != 0).any()
    ref = np.stack([oracle.cgesv_gpu(As[i], bs[i]) for i in range(64)])
    return As, bs, ref, what[:64]


@pytest.mark.parametrize("n", [2, 3, 64])
def test_struct_solve_matches_oracle(batch, n):
    """n = 2: one wave, both halves; n = 3: a lone half; n = 64: the mixed batch.
    The component kernel fills the idle half of a lone half's wave with zeros,
    which no fused level accepts (every key is 0), so that wave reports `redo`
    and the lone system is solved densely: n = 3 checks the hand-over of a
    whole wave, and a lone half on the fused path is covered only by the
    tracker tests below, whose idle slots hold a parked path's system."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_struct_batched
    As, bs, ref, what = batch
    for first in ((0,) if n == 64 else range(0, 64 - n + 1, 7)):
        x = cgesv_struct_batched(As[first:first + n], bs[first:first + n])
        for i in range(n):
            assert same(x[i], ref[first + i]).all(), f"system {first + i} ({what[first + i]}) of a batch of {n}"


def test_struct_solve_covers_the_cases(batch, structure):
    _, _, _, what = batch
    kinds = {w.split()[0] for w in what}
    assert {"jacobian", "random", "tie", "zero", "tiny", "NaN", "inf", "entry"} <= kinds
    # per fused step: a tie inside a triple and, for a 6-row chain, one between its triples
    _, cand, _ = structure
    for step in FUSED:
        pairs = [tuple(int(v) for v in w.split()[2:]) for w in what if w.startswith(f"tie {step} ") and len(w.split()) == 4]
        assert any(a // 3 == b // 3 for a, b in pairs), f"no tie inside a triple at step {step}"
        if len(cand[step]) == 6:
            assert any(a // 3 != b // 3 for a, b in pairs), f"no tie between the triples at step {step}"


def test_entry_outside_the_structure_is_refused(batch, structure):
    import torch
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    _, _, mask = structure
    As, bs, _, _ = batch
    A = As[:4].copy()
    r, c = np.argwhere(~mask)[17]
    A[2, r, c, 1] = 1e-30
    dev = torch.device("cuda:0")
    At, bt = torch.from_numpy(A).to(dev), torch.from_numpy(bs[:4].copy()).to(dev)
    xt = torch.full((4, NV, 2), 7.0, dtype=torch.float32, device=dev)
    st = _abi.lib().hc_cgesv_30x30_struct_batched(4, _abi.ptr(At), _abi.ptr(bt), _abi.ptr(xt),
                                                  _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    assert st == 1, "HC_ERROR_INVALID_VALUE"
    assert (xt.cpu().numpy() == 7.0).all(), "x untouched"


@pytest.mark.parametrize("N", [2, 3])
def test_throughput_kernel_matches_oracle(problem, oracle, samples100, tracker, N):
    """The throughput kernel (never the latency-mode one) at 2 and 3 samples:
    tracks, flags and statistics against the oracle's tracker."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, SMALL_NEVER):
        r = tracker.track(tgt[:N], dif[:N]).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index))
