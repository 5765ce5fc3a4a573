"""expv_taylor_grid without a GPU: the interface, the host-only classification against its restatement, and the numpy restatement of
the whole algorithm (tests/expv_taylor_grid_cases.py) against scipy.linalg.expm on every 64-bit, working-precision case of
tests/test_gpu_expv_taylor_grid.py -- the restatement is the yardstick of the device's parity bar, so it has to be good itself:
at most 128 eps.  Measured: 98.5 eps for the real tridiagonal, n = 257, lin40, alpha = 40 (the worst case, a test of its own below);
65.6 eps worst on the rand13 grids at n <= 257 (random8 Float64, n = 128); 50.3 eps worst at n = 1000 (dense ComplexF64).

The restatement tests need the library only for its theta table and for expv_mi_host_taylor_grid_plan, which every one of them
holds to the classification the restatement used (same_plan): the yardstick and the library must cut the grid the same way."""
import os
import re

import numpy as np
import pytest

from tests import expv_taylor_cases as tc
from tests import expv_taylor_grid_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 128.0
SMALL_N = (1, 5, 63, 64, 65, 127, 128, 129, 257)
WIDE = [np.float64, np.complex128]


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def table(eu):
    return [eu.host_taylor_theta(m, 0) for m in range(1, tc.M_MAX + 1)]


def alpha_for(mk, T):
    return 10.0 if (mk is tc.laplacian and np.dtype(T).kind == "c") else 40.0


def same_plan(eu, info, r):
    """the library classifies the outputs as the restatement did"""
    stage, _, kind = eu.host_taylor_grid_plan(info["s"], r)
    assert [int(x) for x in stage] == info["stage"] and [int(x) for x in kind] == info["kind"]


def test_names_symbols_and_header(eu):
    for name in ("expv_taylor_grid", "expv_taylor_grid_", "host_taylor_grid_plan"):
        assert name in eu.api.__all__ and callable(getattr(eu, name)), name
    lib = eu.api.L.load()
    for sym in ("expv_mi_expv_taylor_grid", "expv_mi_host_taylor_grid_plan"):
        assert sym in eu.api.L.PROTOTYPES and getattr(lib, sym).argtypes is not None, sym
    with open(os.path.join(ROOT, "include", "expv_mi.h")) as f:
        header = f.read()
    decl = re.search(r"int expv_mi_expv_taylor_grid\((.*?)\);", header, re.S).group(1)
    assert "int64_t info[10]" in decl and "double dinfo[4]" in decl and "const double *r, int nt" in decl and "int64_t *col_info" in decl
    assert len(eu.api.L.PROTOTYPES["expv_mi_expv_taylor_grid"][1]) == decl.count(",") + 1
    assert re.search(r"int expv_mi_host_taylor_grid_plan\(int64_t s, const double \*r, int nt, int64_t \*stage, double \*rho, int \*kind\);", header)


@pytest.mark.parametrize("s", [1, 2, 3, 5, 7, 10, 48, 1000])
def test_plan_equals_the_restated_classification(eu, s):
    rng = tc.rng_of(s, 91)
    for R in (1.0, 0.3, 7.25, 1e-3, 1e5):
        ends = np.array([R * i / s for i in range(0, s + 1)])      # the stage ends as floating point computes them
        r = np.concatenate([ends, rng.random(23) * R, [0.0, R, np.nextafter(R, 0.0), 5e-324, R / s * (1 - 2.0 ** -53)]])
        rng.shuffle(r)
        stage, rho, kind = eu.host_taylor_grid_plan(s, r)
        ws, wr, wk = gc.classify(s, r)
        assert np.array_equal(stage, ws) and np.array_equal(kind, wk)
        assert np.array_equal(rho.view(np.uint64), wr.view(np.uint64)), "rho must be the same double"
        assert np.all(rho[kind == 1] >= 0) and np.all(rho[kind == 1] < 1) and np.all(rho[kind == 2] == 1.0)
        assert np.all(stage[kind == 0] == -1) and np.all(stage[kind != 0] >= 0) and np.all(stage < s)
        assert kind[np.flatnonzero(r == R)[0]] == 2 and stage[np.flatnonzero(r == R)[0]] == s - 1


def test_plan_edges(eu):
    stage, rho, kind = eu.host_taylor_grid_plan(4, [])
    assert stage.size == rho.size == kind.size == 0
    stage, rho, kind = eu.host_taylor_grid_plan(4, [0.0, 0.0])      # R = 0: nothing is divided
    assert list(stage) == [-1, -1] and list(kind) == [0, 0] and list(rho) == [0.0, 0.0]
    stage, rho, kind = eu.host_taylor_grid_plan(1, [0.25, 1.0])
    assert list(stage) == [0, 0] and list(kind) == [1, 2] and list(rho) == [0.25, 1.0]
    for bad in ([1.0, -0.5], [float("nan")], [float("inf"), 1.0]):
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.host_taylor_grid_plan(3, bad)
        assert ei.value.kind == "ArgumentError" and "expv_taylor_grid" in str(ei.value)
    with pytest.raises(eu.ExpvMIError):
        eu.host_taylor_grid_plan(0, [1.0])


def test_mixed_signs_are_refused_before_anything_else(eu):
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_grid([0.5, -0.5], None, np.ones(3))
    assert ei.value.kind == "ArgumentError" and "sign" in str(ei.value)


def test_panel_grids_give_the_counts_they_are_built_for(eu):
    for s in (1, 2, 3, 5, 8, 11):
        seen = set()
        for r, counts in gc.panel_grids(s):
            stage, _, kind = eu.host_taylor_grid_plan(s, r)
            got = [int(np.sum((stage == i) & (kind == 1))) for i in range(s)]
            assert got == counts == gc.interior_counts(s, r), (s, got, counts)
            assert kind[-1] == 2 and stage[-1] == s - 1
            seen.update(got)
        assert seen >= set(gc.PANEL_COUNTS) and max(seen) >= 17, (s, seen)


@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.random8], ids=["tridiagonal", "random8"])
def test_restatement_at_R_is_the_single_restatement(table, eu, mk, T):
    tab = [eu.host_taylor_theta(m, tc.table_of(T)) for m in range(1, tc.M_MAX + 1)]
    for n in (5, 129):
        A, b = mk(n, T), tc.vector(n, T)
        t = tc.t_for(A, alpha_for(mk, T), np.dtype(T).kind == "c")
        r = gc.rand13() * 1.75
        mu, alpha, _ = tc.shift_norm(A, r.max() * t)
        W, info = gc.restated_grid(t, r, A, b, T, alpha, tab, tc.TOL[tc.table_of(T)], mu)
        F, single = tc.restated(r.max() * t, A, b, T, alpha, tab, tc.TOL[tc.table_of(T)], mu)
        k = int(np.argmax(r))
        same_plan(eu, info, r)
        assert np.array_equal(np.ascontiguousarray(W[:, k]).view(np.uint8), F.view(np.uint8))
        assert (info["m"], info["s"]) == (single["m"], single["s"]) and info["kind"][k] == 2
        assert np.array_equal(W[:, int(np.argmin(r))], b) and info["kind"][int(np.argmin(r))] == 0
        assert info["applications"] >= single["applications"]


@pytest.mark.parametrize("T", WIDE)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.random8], ids=["tridiagonal", "random8"])
def test_restatement_against_expm_small(table, eu, mk, T):
    worst = 0.0
    for n in SMALL_N:
        A, b = mk(n, T), tc.vector(n, T)
        for ct in ((False, True) if np.dtype(T).kind == "c" else (False,)):
            t = tc.t_for(A, alpha_for(mk, T), ct)
            r = gc.rand13()
            mu, alpha, _ = tc.shift_norm(A, t)
            W, info = gc.restated_grid(t, r, A, b, T, alpha, table, tc.TOL[0], mu)
            same_plan(eu, info, r)
            e = max(gc.relmax_columns(W, gc.truth_columns(A, b, t, r))) / tc.eps_of(T)
            worst = max(worst, e)
            assert e <= CAP, "%s n=%d ct=%s: the restatement is %.1f eps off expm" % (mk.__name__, n, ct, e)
    print("[taylor grid] restatement, n <= 257, %s %s: worst %.1f eps" % (mk.__name__, np.dtype(T).name, worst))


@pytest.mark.parametrize("T", WIDE)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.penta, tc.random8, tc.powerlaw, tc.dense], ids=["tridiagonal", "pentadiagonal", "random8", "powerlaw", "dense"])
def test_restatement_against_expm_n1000(table, eu, mk, T):
    n = 1000
    A, b = mk(n, T), tc.vector(n, T)
    t = tc.t_for(A, alpha_for(mk, T))
    mu, alpha, _ = tc.shift_norm(A, t)
    s = tc.params(alpha, table)[1]
    truths = {}
    for r, L in [(gc.lin40(), 40)] + [(r, s * gc.PANEL_SLOTS) for r, _ in gc.panel_grids(s)]:
        if L not in truths:
            truths[L] = gc.lattice_truth(A, b, t, L)
        W, info = gc.restated_grid(t, r, A, b, T, alpha, table, tc.TOL[0], mu)
        same_plan(eu, info, r)
        e = max(gc.relmax_columns(W, gc.grid_truth(A, b, t, r, L, truths[L]))) / tc.eps_of(T)
        print("[taylor grid] restatement, n = 1000, %s %s q=%d: %.1f eps" % (mk.__name__, np.dtype(T).name, len(r), e))
        assert e <= CAP, "%s q=%d: the restatement is %.1f eps off expm" % (mk.__name__, len(r), e)


def test_the_measured_worst_case_of_the_issue(table, eu):
    """real tridiagonal, n = 257, lin40, alpha = 40, every output against its own expm: 98.5 eps when the scheme was first restated"""
    A, b = tc.laplacian(257, np.float64), tc.vector(257, np.float64)
    t = tc.t_for(A, 40.0)
    mu, alpha, _ = tc.shift_norm(A, t)
    r = gc.lin40()
    W, info = gc.restated_grid(t, r, A, b, np.float64, alpha, table, tc.TOL[0], mu)
    same_plan(eu, info, r)
    e = max(gc.relmax_columns(W, gc.truth_columns(A, b, t, r))) / tc.eps_of(np.float64)
    print("[taylor grid] restatement, tridiagonal n = 257 lin40: %.1f eps" % e)
    assert e <= CAP
