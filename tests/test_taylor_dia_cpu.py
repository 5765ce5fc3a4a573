"""The operators of tests/taylor_dia_cases.py before any device sees them: every case gets the storage form its name says (aliased
narrow band, general diagonal form, SELL slots only), in every element type, and on the 64-bit types the numpy restatements the GPU
tests take their bars from stay within 64 eps of scipy.linalg.expm -- the condition under which `device <= 8 x max(restatement, eps)`
means anything.  No GPU."""
import os

import numpy as np
import pytest
import scipy.linalg as sl

import expv_mi_loader
from tests import expv_taylor_cases as tc
from tests import limits
from tests import phiv_taylor_cases as pc
from tests import taylor_dia_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 64.0
WIDE = [np.float64, np.complex128]


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


def test_the_table_holds_what_the_kernels_need():
    """the remainders of both in-flight loops, both sides of every limit of the analysis, and the offsets the guard is there for"""
    nds = {c.nd for c in dc.CASES if c.form == "aliased"}
    assert {k % 4 for k in nds} == {0, 1, 2, 3} and {k % 2 for k in nds} == {0, 1} and max(nds) == limits.LIMITS["PIPE_DIA_MAX"]
    general = {c.nd for c in dc.CASES if c.form == "general"}
    assert {limits.LIMITS["PIPE_DIA_MAX"] + 1, 13, limits.LIMITS["GDIA_MAX"] - 1, limits.LIMITS["GDIA_MAX"]} <= general
    assert {k % 4 for k in general} == {0, 1, 2, 3}
    assert dc.BY_NAME["nd=33"].form == "sell" and dc.BY_NAME["nd=33"].nd == limits.LIMITS["GDIA_MAX"] + 1
    for offs in (dc.OFFS_31, dc.OFFS_32):
        assert any(o % 2 for o in offs) and max(offs) >= 256 and -min(offs) >= 256 and dc.N_WIDE <= 1000
        assert dc.N_WIDE > 512 and max(offs) > dc.N_WIDE - 512, "rows of the array's first 512-row unit whose column is beyond n"
    assert 0 not in dc.OFFS_ONE_SIDED and min(dc.OFFS_ONE_SIDED) > 0
    for T in dc.DTYPES:
        sh = dc.slice_rows(T)
        for what in ("nd=9", "grid5"):
            got = {dc.BY_NAME["%s n=%s" % (what, k)].operator(T).shape[0] for k in ("SH-1", "SH", "SH+1", "511", "512", "513")}
            assert got == {sh - 1, sh, sh + 1, 511, 512, 513}, (what, T, got)
    assert max(c.operator(np.float64).shape[0] for c in dc.CASES) <= 1000


@pytest.mark.parametrize("T", dc.DTYPES, ids=lambda T: np.dtype(T).name)
@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_every_case_gets_the_form_its_name_says(eu, case, T):
    A = case.operator(T)
    n = A.shape[0]
    assert A.dtype == np.dtype(T) and A.has_sorted_indices
    got = dc.form_of(eu, A, T)
    reordered = dc.stored_ordering(eu, A, T) is not None
    patch = eu.host_patch_order(A, T)[2]["patch_form"]
    print("[taylor dia] %-24s %-10s n=%4d nnz=%6d form %s reordered %s" % (case.name, np.dtype(T).name, n, A.nnz, got, reordered))
    assert got == case.expected(), (case.name, got, case.expected())
    assert len(np.unique(A.indices - np.repeat(np.arange(n), np.diff(A.indptr)))) == case.nd
    if case.form != "sell" or case.nd <= limits.LIMITS["GDIA_MAX"]:
        assert limits.fill_ok(case.nd, n, A.nnz) == (case.form != "sell")
    assert not patch, "a grid wide enough for the patch ordering belongs to the patch test"
    # reverse Cuthill-McKee turns the wrap-around band of a complex type into a narrow one (a default context keeps that ordering);
    # nothing else in the table is reordered: the form above is the form the device stores
    assert reordered == (case.name == "wrap" and np.dtype(T).kind == "c")


def test_the_fill_pair_sits_on_the_rule():
    T = np.float64
    under, over = dc.BY_NAME["nd=32 fill limit"].operator(T), dc.BY_NAME["nd=32 fill limit + 1"].operator(T)
    n = under.shape[0]
    assert under.nnz == over.nnz + 1 and limits.fill_ok(32, n, under.nnz) and not limits.fill_ok(32, n, over.nnz)
    assert limits.source_has(limits.FILL_RULE_SOURCE)
    stored = int(np.count_nonzero(under.diagonal()))
    assert 0.4 * n < stored < 0.6 * n, "the main diagonal is partly stored: mu = tr(A) / n comes from the entries that are there"
    assert 32 * n - under.nnz > 0.2 * 32 * n, "explicit zeros of the form"


def test_the_patch_grid_is_the_smallest_that_takes_the_ordering(eu):
    nx, ny = dc.PATCH_GRID
    for T in dc.DTYPES:
        A = dc.grid5(nx, ny, T)
        perm, _, info = eu.host_patch_order(A, T)
        assert info["patch_form"] and perm is not None and not np.array_equal(perm, np.arange(A.shape[0])), (T, info)
        assert dc.form_of(eu, A, T) == (0, 5, True) and A.shape[0] <= 1000 and dc.stored_ordering(eu, A, T) is None
        assert not eu.host_patch_order(dc.grid5(nx - 1, ny, T), T)[2]["patch_form"]      # rows of 63 cells
        assert not eu.host_patch_order(dc.grid5(nx, 8, T, n=8 * nx - 1), T)[2]["patch_form"]      # fewer than 8 grid rows


@pytest.mark.parametrize("T", WIDE, ids=lambda T: np.dtype(T).name)
@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_restatement_stays_below_64_eps(tables, case, T):
    A = case.operator(T)
    n = A.shape[0]
    b = tc.vector(n, T)
    Ad = A.toarray().astype(tc.wide(T))
    worst, stages = 0.0, None
    for ct in (False, True) if np.dtype(T).kind == "c" else (False,):
        t = tc.t_for(A, case.alpha, ct)
        mu, alpha, _ = tc.shift_norm(A, t)
        Fr, ir = tc.restated(t, A, b, T, alpha, tables[0], tc.TOL[0], mu)
        worst = max(worst, tc.relmax(Fr, sl.expm(t * Ad) @ b) / tc.eps_of(T))
        stages = ir["s"]
        assert ir["s"] >= 2, "several stages: the closing factor and the restart from F are part of every case"
    print("[taylor dia] %-24s %-10s n=%4d s=%d restatement %.1f eps" % (case.name, np.dtype(T).name, n, stages, worst))
    assert worst <= CAP, "%s: %.1f eps" % (case.name, worst)


@pytest.mark.parametrize("T", WIDE, ids=lambda T: np.dtype(T).name)
@pytest.mark.parametrize("case", dc.tagged("phiv"), ids=repr)
def test_augmented_restatement_stays_below_64_eps(tables, case, T):
    A = case.operator(T)
    n = A.shape[0]
    worst = 0.0
    for p in dc.PHIV_PS:
        B = pc.block(n, p, T)
        t = pc.t_for(A, B, case.alpha)
        F, _ = pc.restated(t, A, B, T, tables[0], tc.TOL[0])
        worst = max(worst, tc.relmax(F, pc.truth(t, A, B)) / tc.eps_of(T))
    print("[taylor dia] %-24s %-10s n=%4d phiv restatement %.1f eps" % (case.name, np.dtype(T).name, n, worst))
    assert worst <= CAP, "%s: %.1f eps" % (case.name, worst)
