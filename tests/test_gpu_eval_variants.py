"""The tracking kernels' evaluations alone (include/eval/hc_eval_testing.h):
build_prefixes from the path's own t and sample, the right-hand side by the
stage kinds of the wave's two paths (RHS_MIXED included), dH/dx through the
packed tables read from the workspace or through the slot-absolute tables with
their finiteness verdict, and the evaluations repeated before a dense re-solve,
each against the oracle value for value and against a plain fp64 evaluation of
the raw index tables, at the inputs of tests/eval_cases.py.

Every family is run under eval_cases.arrangement, so that each point family
meets every combination of path slot, own kind and partner (same kind, other
kind, none)."""
import numpy as np
import pytest

import eval_cases as EC
from conftest import same

pytestmark = pytest.mark.gpu

VARIANTS = ("packed", "abs")
TABLES = ("own", "swap_0_9", "owners_helpers")
MAX_LAUNCH = 512
N_PATH = 192


@pytest.fixture(scope="module")
def tabs(problem):
    return EC.tables(problem)


@pytest.fixture(scope="module")
def pool(problem, samples100, oracle):
    """All families in one batch: (points, {family: slice})."""
    thr, band = EC.threshold_points(problem, samples100, oracle)
    fams = [("path", EC.path_points(problem, samples100, N_PATH, 7)), ("scaled", EC.scaled_points(problem, samples100)),
            ("threshold", thr), ("nonfinite", EC.nonfinite_points(problem, samples100))]
    where, at = {}, 0
    for name, p in fams:
        where[name] = slice(at, at + len(p))
        at += len(p)
    return EC.concat([p for _, p in fams]).freeze(), where


@pytest.fixture(scope="module")
def order(pool):
    """The launch order of the pool: every family under its own arrangement
    (partners within the family), the families one after the other."""
    pts, where = pool
    idx, kind = [], []
    for name, sl in where.items():
        i, k = EC.arrangement(sl.stop - sl.start, offset=len(idx) % 5)
        assert EC.coverage(k) == set(EC.COMBOS), name
        idx.append(i + sl.start)
        kind.append(k)
    idx, kind = np.concatenate(idx), np.concatenate(kind)
    assert len(idx) % 8 == 0
    return idx, kind


@pytest.fixture(scope="module")
def refs(problem, oracle, pool, tabs):
    """{table: (p, Hx, ht, h)} of the oracle on the pool, computed once."""
    out = {}
    for name, (dx, dt, _) in tabs.items():
        out[name] = EC.oracle_values(oracle, problem, dx, dt, pool[0])
        for a in out[name]:
            a.setflags(write=False)
    return out


def run(problem, variant, U, pts, idx, kind, redo=False, workspace=None):
    """The hook over an order of points, at most MAX_LAUNCH positions a launch
    (whole workgroups, so a position keeps its slot).  Returns (Hx, rhs,
    ent_ok) per position."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import eval_variant_batched
    assert MAX_LAUNCH % 8 == 0
    out = []
    for a in range(0, len(idx), MAX_LAUNCH):
        i, k = idx[a:a + MAX_LAUNCH], kind[a:a + MAX_LAUNCH]
        out.append(eval_variant_batched(variant, U, pts.x[i], pts.target[i], pts.diff[i], problem.start_params,
                                        pts.t[i], k, redo=redo, workspace=workspace))
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


_results = {}


@pytest.fixture(scope="module")
def results(problem, pool, order, tabs):
    """results(variant, table): the pool under `order`, run once per pair."""
    def get(variant, table):
        if (variant, table) not in _results:
            _results[variant, table] = run(problem, variant, tabs[table][2], pool[0], *order)
        return _results[variant, table]
    yield get
    _results.clear()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def want_rhs(ref, idx, kind):
    _, _, HT, H = ref
    return np.where((kind == 0)[:, None, None], HT[idx], H[idx])


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_bit_exact_against_the_oracle(results, refs, pool, order, variant, table):
    """Every family, every slot / kind / partner combination, each table against
    the oracle on that table: identical values, NaN where the oracle has NaN."""
    idx, kind = order
    HX, RHS, _ = results(variant, table)
    live = kind != EC.IDLE
    want_hx, want_b = refs[table][1][idx], want_rhs(refs[table], idx, kind)
    for name, sl in pool[1].items():
        m = live & (idx >= sl.start) & (idx < sl.stop)
        bad = ~same(HX[m], want_hx[m]).all(axis=(1, 2, 3))
        assert not bad.any(), (name, "dH/dx", np.flatnonzero(m)[bad][:8],
                               np.argwhere(~same(HX[m][bad][0], want_hx[m][bad][0]))[:8])
        bad = ~same(RHS[m], want_b[m]).all(axis=(1, 2))
        assert not bad.any(), (name, "rhs", np.flatnonzero(m)[bad][:8], kind[m][bad][:8],
                               np.argwhere(~same(RHS[m][bad][0], want_b[m][bad][0]))[:8])
    # the non-finite family does hold NaN, and healthy values beside it
    nf = live & (idx >= pool[1]["nonfinite"].start)
    assert np.isnan(HX[nf]).any() and np.isnan(RHS[nf]).any() and np.isfinite(RHS[nf]).any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_within_the_fp64_bound(results, refs, pool, order, tabs, variant):
    """The device values within 32 u S of the plain fp64 evaluation on the finite
    families, the exclusions taken from the reference alone."""
    idx, kind = order
    pts, where = pool
    HX, RHS, _ = results(variant, "own")
    dx, dt, _ = tabs["own"]
    m = (kind != EC.IDLE) & (idx < where["scaled"].stop)
    i, k = idx[m], kind[m]
    ref_hx, ref_ht, ref_h = EC.fp64_values(dx, dt, pts.x[i], refs["own"][0][i], pts.diff[i])
    ref_b = tuple(np.where((k == 0)[:, None], a, b) for a, b in zip(ref_ht, ref_h))
    for name, val, ref in (("dH/dx", HX[m], ref_hx), ("rhs", RHS[m], ref_b)):
        ok, exc, units = EC.bound_check(val, ref)
        print(f"{variant} {name}: worst {units.max():.2f} u, {int(exc.sum())} of {int((ref[1] > 0).sum())} excluded")
        assert ok.all(), (name, np.argwhere(~ok)[:8], units.max())
        assert exc.sum() <= 0.05 * (ref[1] > 0).sum()


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_points_result_is_its_own(problem, samples100, pool, tabs, variant):
    """16 points in every slot, as either kind, beside a partner of the same
    kind, of the other kind, none, a non-finite one and one whose values
    overflow: the same bytes every time (halves contaminating each other, a
    slot-dependent address, RHS_MIXED differing from the pure kinds)."""
    pts, where = pool
    own = pts.take(np.arange(16))
    nf = pts.take(np.arange(where["nonfinite"].start, where["nonfinite"].start + 12))
    huge = EC.huge_partner_points(problem, samples100)
    allp = EC.concat([own, nf, huge])
    per_wave = [[], [], [], []]
    for s in range(8):
        for k in (0, 1):
            for pm in range(5):
                for j in range(16):
                    par = [((j + 1) % 16, k), ((j + 1) % 16, 1 - k), (0, EC.IDLE), (16 + (j + s) % 12, (j + pm) % 2),
                           (28 + (j + s) % 4, (j + k) % 2)][pm]
                    per_wave[s // 2].append(((j, k), par) if s % 2 == 0 else (par, (j, k)))
    idx, kind = [], []
    for g in range(len(per_wave[0])):
        for w in per_wave:
            for i, k in w[g]:
                idx.append(i)
                kind.append(k)
    idx, kind = np.array(idx), np.array(kind, np.uint8)
    HX, RHS, OK = run(problem, variant, tabs["own"][2], allp, idx, kind)
    for j in range(16):
        for k in (0, 1):
            m = np.flatnonzero((idx == j) & (kind == k))
            assert len(m) >= 8 * 5 and set(m % 8) == set(range(8))
            for name, a in (("dH/dx", HX), ("rhs", RHS), ("ent_ok", OK)):
                b = bits(a[m]).reshape(len(m), -1)
                diff = (b != b[0]).any(axis=1)
                assert not diff.any(), (name, j, k, m[diff][:8], np.flatnonzero(b[diff][0] != b[0])[:8])
            # a healthy point keeps its verdict whatever its partner's
            assert (OK[m] == (1 if variant == "abs" else 255)).all()


@pytest.mark.parametrize("table", TABLES)
def test_the_two_variants_agree(results, order, table):
    idx, kind = order
    live = kind != EC.IDLE
    a, b = results("packed", table), results("abs", table)
    assert (bits(a[0][live]) == bits(b[0][live])).all() and (bits(a[1][live]) == bits(b[1][live])).all()


def test_the_finiteness_verdict(results, refs, pool, order, tabs):
    """ABS only.  A lane's verdict covers the (at most six) dH/dx entries it
    computed, of whatever rows: with B entries that must fail it (a component
    not finite or >= 2^64, judged on the oracle's values) at least ceil(B / 6)
    lanes say no; where the six largest entries' squares sum to less than
    2^127 in fp64 every lane says yes; in between it is unconstrained."""
    idx, kind = order
    pts, where = pool
    _, _, OK = results("abs", "own")
    assert (results("packed", "own")[2] == 255).all(), "the packed variant leaves ent_ok untouched"
    live = np.flatnonzero(kind != EC.IDLE)
    assert set(np.unique(OK[live])) <= {0, 1} and (OK[kind == EC.IDLE] == 255).all()
    HXo = refs["own"][1]
    dx, dt, _ = tabs["own"]
    (v, _), _, _ = EC.fp64_values(dx, dt, pts.x, refs["own"][0], pts.diff)
    with np.errstate(all="ignore"):
        sq = np.sort((v.real ** 2 + v.imag ** 2).reshape(len(pts), -1), axis=1)
        must_true = np.isfinite(HXo).all(axis=(1, 2, 3)) & (sq[:, -6:].sum(axis=1) < 2.0 ** 127)
    nbad = np.array([EC.false_entries(A).sum() for A in HXo])
    seen = {"true": 0, "false": 0}
    for pos in live:
        i = idx[pos]
        zeros = int((OK[pos] == 0).sum())
        if nbad[i] > 0:
            assert zeros >= -(-nbad[i] // 6), (pos, i, nbad[i], zeros)
            seen["false"] += 1
        elif must_true[i]:
            assert zeros == 0, (pos, i)
            seen["true"] += 1
    # the low threshold band is all "must be true", the upper two "must be false", and so are the
    # non-finite points whose x[k] a dH/dx term reads (an unknown that enters H linearly only is in no entry)
    t0 = where["threshold"].start
    assert must_true[t0:t0 + 16].all() and (nbad[t0 + 16:t0 + 48] >= 8).all()
    nf_bad = int((nbad[where["nonfinite"]] > 0).sum())
    assert nf_bad >= 30 and must_true[where["path"]].all()
    assert seen["true"] >= N_PATH and seen["false"] >= 32 + nf_bad


@pytest.mark.parametrize("variant", VARIANTS)
def test_redo_returns_the_first_evaluations_values(problem, results, pool, order, tabs, variant):
    """HC_EVAL_REDO: after the entry block was overwritten, the separate
    RHS_HT and RHS_H passes and the second dH/dx give the first evaluation's
    bytes (path, scaled, threshold and non-finite points and partners).  One
    exception, in the right-hand side only: where the first evaluation ran
    RHS_MIXED (acc + (-P) x[w]) and the redo RHS_HT (acc - P x[w]), a NaN comes
    out with the other sign bit (the negation is a source modifier on the NaN
    operand in one and an arithmetic negation in the other); a NaN must still
    meet a NaN, and every other value its own bytes, zeros' signs included."""
    idx, kind = order
    live = kind != EC.IDLE
    first = results(variant, "own")
    again = run(problem, variant, tabs["own"][2], pool[0], idx, kind, redo=True)
    for name, a, b in zip(("dH/dx", "rhs", "ent_ok"), first, again):
        eq = bits(a[live]) == bits(b[live])
        if name == "rhs":
            nan = np.isnan(a[live]) & np.isnan(b[live])
            print(f"{variant}: {int((~eq & nan).sum())} NaN of {int(nan.sum())} differ in their bits")
            eq |= nan
        assert eq.all(), (name, np.argwhere(~eq)[:8], a[live][~eq][:8], b[live][~eq][:8])


def test_against_the_component_evaluation(problem, results, refs, pool, order):
    """hc_trifocal_eval_batched (k_eval: a staged p, LDS copies of the packed
    tables) given the oracle's p(t): the bytes of both variants on the path points."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import eval_batched
    idx, kind = order
    pts, where = pool
    sl = where["path"]
    HX0, HT0, H0 = eval_batched(problem.unified_index, np.array(pts.x[sl]), np.array(refs["own"][0][sl]),
                                np.array(pts.diff[sl]))
    m = (kind != EC.IDLE) & (idx < sl.stop)
    for variant in VARIANTS:
        HX, RHS, _ = results(variant, "own")
        assert (bits(HX[m]) == bits(HX0[idx[m]])).all()
        want = np.where((kind[m] == 0)[:, None, None], HT0[idx[m]], H0[idx[m]])
        assert (bits(RHS[m]) == bits(want)).all()


def test_table_rebuild_under_one_workspace(problem, oracle, ransac0, samples100, pool, refs, tabs):
    """The permuted table, the problem's own and the permuted again through one
    workspace (ABS: the address tables follow the packed ones), each against
    the oracle on its table; a tracking launch on that workspace afterwards
    still matches the oracle."""
    import dataclasses

    import torch

    from checks import SMALL_NEVER, assert_matches_oracle, launch_mode
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker
    tgt, dif, _ = samples100
    N = 2
    tr = DeviceTracker(dataclasses.replace(problem), torch.device("cuda:0"))
    tr.set_ransac_data(ransac0)
    tr.workspace = tr.new_workspace(N)
    ws = tr.workspace.data_ptr()
    pts = pool[0]
    idx, kind = EC.arrangement(48)
    live = kind != EC.IDLE
    for table in ("swap_0_9", "own", "swap_0_9"):
        HX, RHS, _ = run(problem, "abs", tabs[table][2], pts, idx, kind, workspace=tr.workspace)
        assert same(HX[live], refs[table][1][idx][live]).all(), table
        assert same(RHS[live], want_rhs(refs[table], idx, kind)[live]).all(), table
    with launch_mode(tr.L, small=SMALL_NEVER):
        r = tr.track(tgt[:N], dif[:N]).host()
    assert tr.workspace.data_ptr() == ws, "the launches must share one workspace"
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index))


@pytest.mark.parametrize("variant", VARIANTS)
def test_rejected_table_leaves_the_outputs_untouched(problem, pool, variant):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    dev = torch.device("cuda:0")
    pts = pool[0]
    n = 12
    dv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    U = dv(EC.rejected_table(problem), np.int32)
    args = [dv(pts.x[:n], np.float32), dv(pts.target[:n], np.float32), dv(pts.diff[:n], np.float32),
            dv(problem.start_params, np.float32), dv(pts.t[:n], np.float32), dv(np.arange(n) % 2, np.uint8)]
    HX = torch.full((n, 30, 30, 2), 7.0, dtype=torch.float32, device=dev)
    RHS = torch.full((n, 30, 2), 7.0, dtype=torch.float32, device=dev)
    OK = torch.full((n, 32), 7, dtype=torch.uint8, device=dev)
    wsb = int(L.hc_trifocal_workspace_size())
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    p = _abi.ptr
    st = L.hc_trifocal_eval_variant_batched(VARIANTS.index(variant), 0, n, p(U), *(p(a) for a in args), p(HX), p(RHS),
                                            p(OK), p(ws), wsb, p(torch.cuda.current_stream(dev)))
    assert st == 5   # HC_ERROR_TABLE, from the hook itself
    torch.cuda.synchronize(dev)
    assert int(L.hc_trifocal_workspace_status(p(ws))) == 5
    assert (HX == 7.0).all() and (RHS == 7.0).all() and (OK == 7).all()
