"""The four truncated-Taylor entries on wide and many-diagonal operators (tests/taylor_dia_cases.py): the general diagonal form with its
own array, offsets beyond a pack, a slice and a 512-row unit, every remainder of the in-flight loops of csrc/sparse_rows.h, explicit
zeros of the form, the same operators read from SELL slots (dia = 0), the grid-patch ordering, rows without a stored diagonal entry.

Nothing is decided here: every call goes through the `check` of the entry's own test file (tests/test_gpu_expv_taylor.py,
test_gpu_phiv_taylor.py, test_gpu_expv_taylor_grid.py) or the block file's comparison with the single calls, at their bar -- the
device's error <= 8 x max(error of the numpy restatement in the operator's element type, eps_T), relative in the max norm, against
scipy.linalg.expm in fp64 / complex128.  tests/test_taylor_dia_cpu.py holds the restatements of the 64-bit cases to 64 eps and every
case to the storage form its name says.  The figures go to profiles/taylor_dia_parity.txt."""
import os

import numpy as np
import pytest

from tests import expv_taylor_cases as tc
from tests import expv_taylor_grid_cases as gc
from tests import phiv_taylor_cases as pc
from tests import taylor_dia_cases as dc
from tests import test_gpu_expv_taylor as single
from tests import test_gpu_expv_taylor_block as blk
from tests import test_gpu_expv_taylor_grid as grid
from tests import test_gpu_phiv_taylor as phiv
from tests.option_forms import context_with

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lines = {"expv_taylor": [], "phiv_taylor": [], "expv_taylor_grid": []}
HEADERS = {      # (the column layouts of the three files whose `check` writes the lines)
    "expv_taylor": "%-44s %-10s %4s %8s %3s %4s %6s %5s %10s %10s %10s" % ("case", "dtype", "prec", "alpha", "m*", "s", "apps", "path", "restated", "device", "expm_mult"),
    "phiv_taylor": "%-40s %-10s %2s %8s %3s %4s %6s %5s %9s %9s %10s %10s" % ("case", "dtype", "p", "alpha", "m*", "s", "apps", "path", "nu", "U", "restated", "device"),
    "expv_taylor_grid": "%-40s %-10s %4s %7s %3s %3s %4s %4s %5s %5s %5s %4s %10s %10s %6s" % ("case", "dtype", "prec", "alpha", "m*", "s", "q", "qmax", "apps", "terms", "accum",
                                                                                                 "path", "restated", "device", "gap"),
}
_notes = []
_lattices = {}
TYPE_IDS = dict(ids=lambda T: np.dtype(T).name)
DIA_CASES = [c for c in dc.CASES if c.form != "sell"]
NCOLS = (2, 3, 8, 9)      # panels of 2 (the 16-byte-row types) / 4, 4, 8, 8 + a remainder panel of one column


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


@pytest.fixture(scope="module")
def ctx_dia0(eu):
    return context_with(eu, {"dia": 0})


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    if not any(_lines.values()):
        return
    try:
        with open(os.path.join(ROOT, "profiles", "taylor_dia_parity.txt"), "w") as f:
            f.write("# The truncated-Taylor entries on the operators of tests/taylor_dia_cases.py against scipy.linalg.expm: relative max-norm errors;\n"
                    "# bar = 8 x max(restatement, eps).  The columns of each part are those of the entry's own table (expv_taylor_parity.txt,\n"
                    "# phiv_taylor_parity.txt, expv_taylor_grid_parity.txt); the case names carry the storage form and the context.\n")
            for entry, lines in _lines.items():
                f.write("\n## %s\n%s\n" % (entry, HEADERS[entry]) + "\n".join(lines) + "\n")
            f.write("\n## forms and counts\n" + "\n".join(_notes) + "\n")
    except OSError:
        pass


def through(mod, entry, fn, *args, **kw):
    """fn(*args, **kw) of another test file; the lines it adds to that file's parity table are moved to this one's"""
    k0 = len(mod._lines)
    try:
        return fn(*args, **kw)
    finally:
        _lines[entry].extend(mod._lines[k0:])
        del mod._lines[k0:]


def bits(x):
    return np.ascontiguousarray(np.asarray(x)).view(np.uint8)


def label(case):
    """the case's name with the storage form its operator takes"""
    pipe, gen, _ = case.expected()
    return "%s [%s]" % (case.name, "aliased %d" % pipe if pipe else "general %d" % gen if gen else "sell %d" % case.nd)


def operator(eu, case, T, ctx=None):
    """(A, op): the operator of a case on the default (or the given) context, with the stored form asserted"""
    A = case.operator(T)
    op = eu.MIOperator(A) if ctx is None else eu.MIOperator(A, ctx)
    reordered = bool(op.reorder_info["reordered"])
    # (tests/test_taylor_dia_cpu.py: reverse Cuthill-McKee narrows the wrap-around band of a complex type, nothing else is reordered)
    assert reordered == (case.name == "wrap" and np.dtype(T).kind == "c"), (case.name, T, op.reorder_info)
    if not reordered:
        assert dc.form_of(eu, A, T) == case.expected(), (case.name, T)
    return A, op


def ts_of(case, A, T):
    return [tc.t_for(A, case.alpha, ct) for ct in single.t_variants(T)]


def key_of(case, T, t):
    return ("taylor dia", case.name, np.dtype(T).name, complex(t))


# ---- expv_taylor: every case, every type, and the same numbers from SELL slots ----------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_expv_taylor_on_every_form(eu, tables, ctx_dia0, case, T):
    A, op = operator(eu, case, T)
    n = A.shape[0]
    b = tc.vector(n, T)
    op0 = operator(eu, case, T, ctx_dia0)[1] if case.form != "sell" else None
    for t in ts_of(case, A, T):
        w, info = through(single, "expv_taylor", single.check, eu, tables, label(case), A, b, t, op=op, path=1, key=key_of(case, T, t))
        if op0 is None:
            continue
        # csrc/sparse_rows.h: both forms sum a row in ascending column order, the diagonal form adds exact zeros only
        w0, info0 = eu.expv_taylor(t, op0, b, return_info=True)
        assert info0 == info, (info0, info)
        assert np.all(np.isfinite(np.asarray(w))) and np.array_equal(np.asarray(w0), np.asarray(w)), \
            "%s %s: dia = 0 differs by %.3e" % (case.name, np.dtype(T).name, tc.relmax(np.asarray(w0), np.asarray(w)))
    _notes.append("expv_taylor       %-28s %-10s n=%4d nd=%2d Q=4 remainder %d%s" % (label(case), np.dtype(T).name, n, case.nd, case.nd % 4,
                                                                                  "" if op0 is None else "  == dia 0 (SELL slots)"))


# ---- expv_taylor_block: panels of 2 / 4 / 8 columns and a remainder panel ----------------------------------------------------------
def block_of(n, T):
    """9 columns: 0.001 x random, zero, random ... -- the columns stop at different terms, one never starts"""
    T = np.dtype(T)
    B = np.empty((n, max(NCOLS)), dtype=T, order="F")
    for k in range(B.shape[1]):
        B[:, k] = tc.vector(n, T, seed=k)
    B[:, 0] *= T.type(0.001)
    B[:, 1] = 0.0
    return B


@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
@pytest.mark.parametrize("case", dc.tagged("block"), ids=repr)
def test_block_columns_equal_their_single_calls(eu, case, T):
    A, op = operator(eu, case, T)
    n = A.shape[0]
    B = block_of(n, T)
    t = tc.t_for(A, case.alpha)
    refs = [blk.single_ref(eu, t, op, B[:, k]) for k in range(B.shape[1])]
    assert refs[1][1][0] == 0 and max(r[1][0] for r in refs) > 0, "a column that never starts beside columns that run: %r" % ([r[1] for r in refs],)
    for p in NCOLS:
        Bp = np.asfortranarray(B[:, :p])
        W, info = eu.expv_taylor_block(t, op, Bp, return_info=True)
        blk.assert_equals_singles(eu, t, op, Bp, W, info, refs=refs)
        blk.assert_block_path(info, p)
    _notes.append("expv_taylor_block %-28s %-10s n=%4d nd=%2d p=%s: every column == its single call" % (label(case), np.dtype(T).name, n, case.nd, NCOLS))


# ---- expv_taylor_grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
@pytest.mark.parametrize("case", dc.tagged("grid"), ids=repr)
def test_time_grid_outputs(eu, tables, case, T):
    A, op = operator(eu, case, T)
    n = A.shape[0]
    b = tc.vector(n, T)
    t = tc.t_for(A, case.alpha)
    s = tc.params(tc.shift_norm(A, t)[1], tables[tc.table_of(T, 0)])[1]
    L = s * gc.PANEL_SLOTS
    lat = _lattices.setdefault((case.name, np.dtype(T).name), gc.lattice_truth(A, b, t, L))
    single_w = np.asarray(eu.expv_taylor(t, op, b))
    # five outputs (three inside stages, b itself, the end), and the grid of expv_taylor_grid_cases with the most outputs in one stage:
    # more than one panel of eight
    five = np.array([7, L // 2 + 3, L, 0, L - 7], dtype=np.float64) / L      # (no multiple of PANEL_SLOTS but L: inside their stages)
    wide_r, counts = max(gc.panel_grids(s), key=lambda g: max(g[1]))
    assert max(counts) > 8
    for gname, r in (("five", five), ("panels", wide_r)):
        W, info = through(grid, "expv_taylor_grid", grid.check, eu, tables, "%s %s" % (label(case), gname), A, b, t, r, gc.grid_truth(A, b, t, r, L, lat),
                          op=op, path=1, gap=lat[1])
        ends = np.flatnonzero(r == 1.0)
        assert ends.size >= 1 and sum(k == 1 for k in info["kind"]) >= 3
        for k in ends:
            assert info["kind"][k] == 2 and np.array_equal(bits(W[:, k]), bits(single_w)), "the output at R is not the single call's result"
    _notes.append("expv_taylor_grid  %-28s %-10s n=%4d nd=%2d outputs 5 and %d (up to %d in a stage)" % (label(case), np.dtype(T).name, n, case.nd, wide_r.size,
                                                                                                     max(counts)))


# ---- phiv_taylor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
@pytest.mark.parametrize("case", dc.tagged("phiv"), ids=repr)
def test_phiv_taylor(eu, tables, case, T):
    A, op = operator(eu, case, T)
    n = A.shape[0]
    for p in dc.PHIV_PS:
        B = pc.block(n, p, T)
        through(phiv, "phiv_taylor", phiv.check, eu, tables, label(case), A, B, pc.t_for(A, B, case.alpha), op=op, path=1,
                key=("taylor dia", case.name, np.dtype(T).name, p))
    _notes.append("phiv_taylor       %-28s %-10s n=%4d nd=%2d p=%s" % (label(case), np.dtype(T).name, n, case.nd, dc.PHIV_PS))


# ---- grid-patch ordering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
def test_grid_patch_ordering_answers_in_the_callers_ordering(eu, tables, T):
    nx, ny = dc.PATCH_GRID
    A = dc.grid5(nx, ny, T)
    n = A.shape[0]
    b = tc.vector(n, T)
    t = tc.t_for(A, 40.0)
    key = ("taylor dia", "patch grid", np.dtype(T).name, complex(t))
    op = eu.MIOperator(A)
    assert op.patch_info["patch_form"] and op.patch_info["grid_row_length"] == nx and op.reorder_info["reordered"], (op.patch_info, op.reorder_info)
    w, info = through(single, "expv_taylor", single.check, eu, tables, "grid5 %dx%d [patch ordering]" % (nx, ny), A, b, t, op=op, path=1, key=key)
    # the same matrix in its natural ordering: the general diagonal form, the same bar
    ctx0 = context_with(eu, {"patch": 0})
    op0 = eu.MIOperator(A, ctx0)
    assert not op0.patch_info["patch_form"] and not op0.reorder_info["reordered"]
    assert eu.host_pattern_info(A, T)["general_dia_diagonals"] == 5
    through(single, "expv_taylor", single.check, eu, tables, "grid5 %dx%d [general 5, patch 0]" % (nx, ny), A, b, t, op=op0, path=1, key=key)
    # (the truth is in the caller's ordering: an answer left in the stored one is O(1) away from it)
    B =np.asfortranarray(block_of(n, T)[:, :3])
    B[:, 0] = b
    W, binfo = eu.expv_taylor_block(t, op, B, return_info=True)
    blk.assert_equals_singles(eu, t, op, B, W, binfo)
    blk.assert_block_path(binfo, 3)
    assert np.array_equal(bits(np.asarray(W)[:, 0]), bits(w))
    _notes.append("expv_taylor(+block p=3) grid5 %dx%d %-10s n=%4d patch ordering, %d tiles" % (nx, ny, np.dtype(T).name, n, op.patch_info["tiles"]))


# ---- born on the device from diagonals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
def test_operator_from_diagonals_gives_the_same_bits(eu, T):
    (case,) = dc.tagged("from_dia")
    ctx = eu.Context()
    A, op = operator(eu, case, T, ctx)
    n = A.shape[0]
    D = A.todia()
    assert len(D.offsets) == case.nd and A.nnz == sum(n - abs(int(o)) for o in D.offsets), "full diagonals: from_dia stores the same pattern"
    opd = eu.MIOperator.from_dia(D, ctx=ctx)
    b = tc.vector(n, T)
    for t in ts_of(case, A, T):
        w, info = eu.expv_taylor(t, op, b, return_info=True)
        wd, infod = eu.expv_taylor(t, opd, b, return_info=True)
        assert info["path"] == 1 and infod == info, (infod, info)
        assert np.array_equal(bits(wd), bits(w))


# ---- non-finite input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float64, np.complex64], **TYPE_IDS)
@pytest.mark.parametrize("case", dc.tagged("inf"), ids=repr)
def test_an_infinite_entry_is_returned_not_raised(eu, tables, case, T):
    A, op = operator(eu, case, T)
    n = A.shape[0]
    b = tc.vector(n, T)
    t = tc.t_for(A, case.alpha)
    bad = b.copy()
    bad[n // 3] = np.inf
    w, info = eu.expv_taylor(t, op, bad, return_info=True)
    assert info["nonfinite_stage"] >= 1 and not np.all(np.isfinite(np.asarray(w))) and not np.isfinite(info["normF"])
    assert info["applications"] < info["launches"] or info["s"] == 1
    through(single, "expv_taylor", single.check, eu, tables, label(case) + " after inf", A, b, t, op=op, path=1, key=key_of(case, T, t))


# ---- mu and alpha from rows without a stored diagonal entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES, **TYPE_IDS)
@pytest.mark.parametrize("case", dc.tagged("mu"), ids=repr)
def test_shift_and_norm(eu, case, T):
    A, op = operator(eu, case, T)
    n = A.shape[0]
    t = tc.t_for(A, case.alpha)
    mu, alpha, longest = tc.shift_norm(A, t)
    _, info = eu.expv_taylor(t, op, tc.vector(n, T), return_info=True)
    d = A.diagonal().astype(tc.wide(T))
    stored = int(np.count_nonzero(d))
    # alpha: the tolerance of tests/test_gpu_expv_taylor.py's check; mu: a sum of n terms in any order, (n - 1) u sum |d_i|, and a division
    assert abs(info["alpha"] - alpha) <= 4 * longest * tc.eps_of(np.float64) * alpha, (info["alpha"], alpha)
    assert abs(info["mu"] - mu) <= n * tc.eps_of(np.float64) * float(np.abs(d).sum()) / n, (info["mu"], mu)
    if case.name == "one-sided":
        assert stored == 0 and info["mu"] == 0 and mu == 0
    else:
        assert 0 < stored <= n and abs(mu) > 0.1
    _notes.append("k_taylor_shift_norm %-26s %-10s n=%4d stored diagonal entries %4d mu %.6g alpha %.6g" % (case.name, np.dtype(T).name, n, stored,
                                                                                                        abs(info["mu"]), info["alpha"]))
