"""exp(tA)b for a REAL operator with a complex time and complex vectors on the device (expv_mi_expv_taylor_realop,
eu.expv_taylor_realop).

Truth for values: scipy.linalg.expm(tA) b in complex128 (n <= 1000).  Bar, as in tests/test_gpu_expv_taylor.py: the device's error
<= 8 x max(error of the numpy restatement run in the operator's complex type on the same input, eps_C), both relative in the max norm
-- the device differs from the restatement only in the summation order inside a row and in FMA contraction.  On an operator with a
fused form the call is also compared, element for element with ==, with expv_taylor on the operator promoted to the complex type: the
rounding contract of include/expv_mi.h.  Every case's figures go to profiles/expv_taylor_realop_parity.txt.

The 2-D grid in patch order: the patch ordering permutes the rows and keeps the SELL slots, so taylor_fused() holds for it and the
call reports the fused path (tests/test_gpu_taylor_dia.py asserts the same of expv_taylor).  Its tiles are sized by the element
type, so the promoted operator is stored in ANOTHER ordering, a row's entries are summed in another order there, and the two calls
differ by rounding (1.2e-14 at n = 1000 in Float64): the test asserts the ordering, the fused path and the bar, not ==."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests import expv_taylor_cases as tc
from tests import expv_taylor_realop_cases as rc
from tests import taylor_dia_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = rc.BAR
_records, _truths, _small = [], {}, {}


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    if not _records:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "expv_taylor_realop_parity.txt"), "w") as f:
            f.write("# expv_taylor_realop against scipy.linalg.expm(tA) b (n = 70001: against scipy's expm_multiply): relative max-norm errors; "
                    "bar = 8 x max(restatement, eps); '==': equal, element for element, to expv_taylor on the promoted operator (-: not compared)\n")
            f.write("%-40s %-8s %4s %8s %3s %4s %6s %5s %10s %10s %3s\n" % ("case", "R", "prec", "alpha", "m*", "s", "apps", "path", "restated", "device", "=="))
            for r in _records:
                f.write("%-40s %-8s %4d %8.3f %3d %4d %6d %5d %10.2e %10.2e %3s\n" % (r["case"], r["R"], r["precision"], r["alpha"], r["m"], r["s"], r["apps"],
                                                                                     r["path"], r["restated"], r["device"], r.get("eq", "-")))
    except OSError:
        pass


def as_dense(A):
    return (A.toarray() if sp.issparse(A) else np.asarray(A)).astype(np.complex128)


def truth_of(key, A, b, t):
    if key not in _truths:
        _truths[key] = sl.expm(t * as_dense(A)) @ b.astype(np.complex128)
    return _truths[key]


def check(eu, tables, name, A, b, t, precision=0, op=None, path=1, opnorm=None, truth=None, truth_bar=None):
    """one call of the device against the restatement and the truth; returns (w, info, record)"""
    R = np.dtype(A.dtype)
    Cd = rc.complex_of(R)
    mu, alpha, longest, tab, Fr, ir = rc.plan_and_restatement(A, b, t, tables, precision, opnorm)
    if truth is None:
        truth = truth_of((name, R.name, A.shape[0], complex(t), b.dtype.name), A, b, t)
    w, info = eu.expv_taylor_realop(t, A if op is None else op, b, precision=precision, opnorm=opnorm, return_info=True)
    w = np.asarray(w)
    assert w.dtype == Cd and w.shape == b.shape
    assert eu.expv_taylor_realop.last_info == info
    e_rest, e_dev = tc.relmax(Fr, truth), tc.relmax(w, truth)
    rec = {"case": "%s n=%d" % (name, A.shape[0]), "R": R.name, "precision": precision, "alpha": info["alpha"], "m": info["m"], "s": info["s"],
           "apps": info["applications"], "path": info["path"], "restated": e_rest, "device": e_dev}
    _records.append(rec)
    print("[taylor realop]", rec)
    # norm and parameters
    assert abs(info["alpha"] - alpha) <= 4 * longest * tc.eps_of(np.float64) * alpha, (info["alpha"], alpha)
    assert (info["m"], info["s"]) == eu.host_taylor_params(info["alpha"], tab)
    assert (info["m"], info["s"]) == (ir["m"], ir["s"])
    # the stopping rule: at most one borderline stop per stage away from the restatement; never a blocking read per term
    assert abs(info["applications"] - ir["applications"]) <= info["s"], (info, ir)
    assert info["launches"] == info["m"] * info["s"] and info["host_reads"] <= 2, info
    assert info["nonfinite_stage"] == 0
    assert info["path"] == path, info
    # values
    if R == np.float64 and precision == 0 and truth_bar is None:
        assert e_rest <= 64 * tc.eps_of(Cd), "the 64-bit cases are chosen so that the restatement stays below 64 eps: %.2e" % e_rest
    bar = BAR * max(e_rest if truth_bar is None else truth_bar, tc.eps_of(Cd))
    assert e_dev <= bar, "%s: device %.3e > %g x max(restatement %.3e, eps)" % (name, e_dev, BAR, e_rest if truth_bar is None else truth_bar)
    return w, info, rec


def assert_equals_promoted(eu, A, b, t, w, info, rec, op_promoted=None, precision=0):
    """the rounding contract: == the single call on the operator promoted to the complex type, whenever that call is fused too"""
    Cd = rc.complex_of(A.dtype)
    wp, ip = eu.expv_taylor(t, A.astype(Cd) if op_promoted is None else op_promoted, b.astype(Cd), precision=precision, return_info=True)
    if ip["path"] != 1:
        return False
    eq = bool(np.array_equal(w, np.asarray(wp)))
    rec["eq"] = "yes" if eq else "NO"
    for k in ("alpha", "m", "s", "applications"):
        assert info[k] == ip[k], (k, info, ip)
    assert eq, "fused realop differs from the promoted call: max |diff| = %.3e" % float(np.max(np.abs(w - np.asarray(wp))))
    return True


def small(eu, tables, case, R, n):
    key = (case[0], np.dtype(R).name, n)
    if key not in _small:
        name, mk, alpha, t_of = case
        A, b = mk(n, R), rc.cvector(n, R)
        t = t_of(A, alpha)
        _small[key] = (A, b, t) + check(eu, tables, name, A, b, t, path=1)
    return _small[key]


# ---- 1. slice and pack boundaries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.SMALL_N)
@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("case", rc.SMALL_CASES, ids=rc.CASE_IDS)
def test_slice_and_pack_boundaries(eu, tables, case, R, n):
    small(eu, tables, case, R, n)


# ---- 2. the rounding contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.SMALL_N)
@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("case", rc.SMALL_CASES, ids=rc.CASE_IDS)
def test_fused_path_equals_the_promoted_operator_element_for_element(eu, tables, case, R, n):
    A, b, t, w, info, rec = small(eu, tables, case, R, n)
    assert assert_equals_promoted(eu, A, b, t, w, info, rec), "the promoted operator of these cases has a fused form"


# ---- 3. every operator form at n = 1000 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("mk,path,t_of,alpha", [(tc.laplacian, 1, rc.schroedinger_t, 10.0), (tc.penta, 1, rc.ray_t, 40.0), (tc.random8, 1, rc.ray_t, 40.0),
                                                (tc.powerlaw, 2, rc.ray_t, 40.0), (tc.dense, 2, rc.ray_t, 40.0)],
                         ids=["tridiagonal", "pentadiagonal", "random8", "powerlaw", "dense"])
def test_n1000_every_operator_form(eu, tables, mk, path, t_of, alpha, R):
    n = 1000
    A, b = mk(n, R), rc.cvector(n, R)
    t = t_of(A, alpha)
    op = eu.MIOperator(A)
    before = op.ctx.counters()["op_applies"]
    w, info, rec = check(eu, tables, mk.__name__, A, b, t, op=op, path=path)
    applied = op.ctx.counters()["op_applies"] - before
    assert applied == (1 if path == 1 else 2) * info["launches"], "path 2 applies the operator to the real and to the imaginary plane"
    if path == 1:
        assert assert_equals_promoted(eu, A, b, t, w, info, rec)


@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_grid_in_patch_order(eu, tables, R):
    nx, ny = dc.PATCH_GRID
    n = 1000
    A, b = dc.grid5(nx, ny + 1, R, n=n), rc.cvector(n, R)
    t = rc.schroedinger_t(A, 10.0)
    op = eu.MIOperator(A)
    assert op.patch_info["patch_form"] and op.patch_info["grid_row_length"] == nx and op.reorder_info["reordered"], (op.patch_info, op.reorder_info)
    # (the truth is in the caller's ordering: an answer left in the stored one is O(1) away from it)
    w, info, rec = check(eu, tables, "grid5 %dx%d [patch order]" % (nx, ny + 1), A, b, t, op=op, path=1)
    # the same matrix in its natural ordering, where the promoted operator is stored in the same order: the general diagonal form, ==
    ctx0 = eu.Context()
    ctx0.set_option("patch", 0)
    op0 = eu.MIOperator(A, ctx0)
    assert not op0.patch_info["patch_form"] and not op0.reorder_info["reordered"]
    w0, info0, rec0 = check(eu, tables, "grid5 %dx%d [natural order]" % (nx, ny + 1), A, b, t, op=op0, path=1)
    assert assert_equals_promoted(eu, A, b, t, w0, info0, rec0, op_promoted=eu.MIOperator(A.astype(rc.complex_of(R)), ctx0))


@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_reordered_operator_answers_in_the_callers_ordering(eu, tables, R):
    n = 1000
    ctx = eu.Context()
    ctx.set_option("reorder", 2)      # always keep the bandwidth-reducing ordering
    A, _ = tc.shuffled_band(n, R)
    A.sort_indices()
    op = eu.MIOperator(A, ctx)
    ri = op.reorder_info
    assert ri["reordered"] and ri["bandwidth_after"] < ri["bandwidth_before"], ri
    b = rc.cvector(n, R)
    t = rc.ray_t(A, 40.0)
    w, info, rec = check(eu, tables, "shuffled band", A, b, t, op=op, path=1)
    assert_equals_promoted(eu, A, b, t, w, info, rec, op_promoted=op.astype(rc.complex_of(R)))
    # a real b takes the same way in: permuted in its own type, widened behind it
    br = tc.vector(n, R)
    assert np.array_equal(np.asarray(eu.expv_taylor_realop(t, op, br)), np.asarray(eu.expv_taylor_realop(t, op, br.astype(rc.complex_of(R)))))


@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_matrix_free_operator_sees_real_vectors_twice_per_term(eu, torch, tables, R):
    n = 1000
    A, b = tc.penta(n, R), rc.cvector(n, R)
    Ad = torch.as_tensor(A.toarray()).cuda()
    torch.cuda.synchronize()
    seen = []

    def matvec(x):
        seen.append((x.dtype, x.numel()))
        return Ad @ x
    ctx = eu.Context()
    op = eu.MIOperator(None, ctx, matvec=matvec, shape=(n, n), dtype=R, ishermitian=False)
    opnorm = float(abs(A).sum(axis=1).max())
    t = -1j * 10.0 / opnorm
    w, info, _ = check(eu, tables, "matrix-free", A, b, t, op=op, path=2, opnorm=opnorm)
    assert len(seen) == 2 * info["launches"] and ctx.counters()["op_applies"] == len(seen), (len(seen), info)
    assert set(seen) == {(Ad.dtype, n)}, "the callback's contract: real vectors of n elements"
    wv = np.full(n, 7 + 7j, dtype=rc.complex_of(R))
    with pytest.raises(eu.ExpvMIError) as ei:      # a callback without its bound
        eu.expv_taylor_realop_(wv, t, op, b)
    assert ei.value.kind == "ArgumentError" and "opnorm" in str(ei.value) and np.all(wv == 7 + 7j)


# ---- 4. a real b -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("mk,path", [(tc.penta, 1), (tc.powerlaw, 2)], ids=["fused", "update"])
def test_real_b_is_widened_on_the_device(eu, torch, tables, mk, path, R):
    n = 257
    Cd = rc.complex_of(R)
    A, b = mk(n, R), tc.vector(n, R)
    op = eu.MIOperator(A)
    t = rc.schroedinger_t(A, 10.0)
    w, info, _ = check(eu, tables, mk.__name__ + " real b", A, b, t, op=op, path=path)
    want = np.asarray(eu.expv_taylor_realop(t, op, b.astype(Cd)))
    assert np.array_equal(w.view(np.uint8), want.view(np.uint8)), "a real b on the host: other bits than b.astype(complex)"
    wd = eu.expv_taylor_realop(t, op, torch.as_tensor(b).cuda())
    assert torch.is_tensor(wd) and wd.is_cuda and wd.dtype == (torch.complex64 if R == np.float32 else torch.complex128)
    assert np.array_equal(wd.cpu().numpy().view(np.uint8), want.view(np.uint8)), "a real b on the device"
    x = torch.as_tensor(b.astype(Cd)).cuda()
    assert eu.expv_taylor_realop_(x, t, op, x) is x      # w aliases a complex b
    assert np.array_equal(x.cpu().numpy().view(np.uint8), want.view(np.uint8)), "aliased device vectors: other bits than with separate ones"
    assert eu.expv_taylor_realop.last_info == info


# ---- 5. many workgroups --------------------------------------------------------------------------------------------------------------------
def test_more_workgroups_than_compute_units(eu, tables):
    """n = 70 001: the ticket's last arrival is not the last workgroup launched.  Values against scipy's expm_multiply on the CPU; bar
    from its own agreement with the restatement."""
    n = 70001
    A, b = tc.penta(n, np.float64), rc.cvector(n, np.float64)
    t = rc.ray_t(A, 40.0)
    ref = spl.expm_multiply(t * A, b)
    Fr = rc.plan_and_restatement(A, b, t, tables)[4]
    w, info, rec = check(eu, tables, "penta", A, b, t, path=1, truth=ref, truth_bar=tc.relmax(Fr, ref))
    assert assert_equals_promoted(eu, A, b, t, w, info, rec)


# ---- 6. the 2^-24 table on a Float64 operator ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.SMALL_CASES, ids=rc.CASE_IDS)
def test_precision_1_on_a_float64_operator(eu, tables, case):
    n = 257
    name, mk, alpha, t_of = case
    A, b = mk(n, np.float64), rc.cvector(n, np.float64)
    t = t_of(A, alpha)
    w, info, rec = check(eu, tables, name, A, b, t, precision=1, path=1)
    assert (info["m"], info["s"]) == eu.host_taylor_params(info["alpha"], 1) and info["m"] * info["s"] < _small_need(eu, tables, case, n)
    assert assert_equals_promoted(eu, A, b, t, w, info, rec, precision=1)


def _small_need(eu, tables, case, n):
    info = small(eu, tables, case, np.float64, n)[4]
    return info["m"] * info["s"]


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_t_zero_returns_b_bit_for_bit(eu, R):
    n = 129
    A, b = tc.random8(n, R), rc.cvector(n, R)
    for t in (0.0, 0j):
        w, info = eu.expv_taylor_realop(t, A, b, return_info=True)
        assert np.array_equal(np.asarray(w).view(np.uint8), b.view(np.uint8))
        assert (info["m"], info["s"], info["applications"], info["launches"], info["alpha"]) == (0, 1, 0, 0, 0.0)


@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_real_time_acts_on_both_planes(eu, tables, R):
    """t_im = 0: exp(tA) applied to Re b and Im b.  The two real calls round F + c v once (one fused multiply-add), the complex
    element step twice, and they stop on other maxima: the three results agree within the bar, not bit for bit."""
    n = 257
    Cd = rc.complex_of(R)
    A, b = tc.penta(n, R), rc.cvector(n, R)
    t = tc.t_for(A, 20.0)
    w, info, rec = check(eu, tables, "penta real t", A, b, t, path=1)
    planes = np.asarray(eu.expv_taylor(t, A, np.ascontiguousarray(b.real))) + 1j * np.asarray(eu.expv_taylor(t, A, np.ascontiguousarray(b.imag)))
    assert tc.relmax(w, planes.astype(Cd)) <= BAR * max(rec["restated"], tc.eps_of(Cd))


@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_zero_vector_costs_no_application(eu, R):
    n = 257
    A = tc.random8(n, R)
    for b in (np.zeros(n, dtype=rc.complex_of(R)), np.zeros(n, dtype=R)):
        w, info = eu.expv_taylor_realop(rc.ray_t(A, 40.0), A, b, return_info=True)
        assert not np.any(np.asarray(w)) and info["applications"] == 0 and info["launches"] == info["m"] * info["s"] > 0
        assert info["normF"] == 0.0 and info["nonfinite_stage"] == 0


@pytest.mark.parametrize("R", rc.REALS, ids=["f64", "f32"])
def test_zero_operator_returns_b(eu, R):
    n = 129
    b = rc.cvector(n, R)
    Z = (sp.identity(n, format="csr") * 0.0).astype(R)      # (n stored zeros)
    assert Z.nnz == n and not Z.data.any()
    w, info = eu.expv_taylor_realop(0.5 - 2j, Z, b, return_info=True)
    assert np.array_equal(np.asarray(w).view(np.uint8), b.view(np.uint8))
    assert info["alpha"] == 0.0 and (info["m"], info["s"], info["applications"]) == (0, 1, 0)


def test_empty_operator_does_nothing(eu):
    h = C.c_void_p()
    ctx = eu.default_context()
    lib = eu.api.L.load()
    rp = np.zeros(1, dtype=np.int32)
    eu.api._check(lib.expv_mi_op_create_csr(ctx._h, eu.api.L.F64, 0, rp.ctypes.data, None, None, 4, 0, C.byref(h)), ctx._h)
    try:
        info, dinfo = (C.c_int64 * 8)(*([7] * 8)), (C.c_double * 4)(*([7.0] * 4))
        eu.api._check(lib.expv_mi_expv_taylor_realop(ctx._h, h, 0.0, 1.0, None, 0, eu.api.L.C64, None, 0, 0, 0, 0.0, info, dinfo), ctx._h)
        assert list(info) == [0] * 8 and list(dinfo) == [0.0] * 4
    finally:
        lib.expv_mi_op_destroy(h)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_w_untouched(eu):
    n = 257
    A, b = tc.penta(n, np.float64), rc.cvector(n, np.float64)
    t = rc.ray_t(A, 40.0)
    op = eu.MIOperator(A)
    _, info = eu.expv_taylor_realop(t, op, b, return_info=True)
    need = info["m"] * info["s"]
    w = np.full(n, 7 + 7j)

    def refused(call):
        with pytest.raises(eu.ExpvMIError) as ei:
            call()
        assert ei.value.kind == "ArgumentError", ei.value
        assert np.all(w == 7 + 7j), "a refused call must leave w alone"
        return str(ei.value)
    msg = refused(lambda: eu.expv_taylor_realop_(w, t, eu.MIOperator(A.astype(np.complex128)), b))
    assert "expv_taylor_realop" in msg and "expv_mi_expv_taylor" in msg, msg
    refused(lambda: eu.expv_taylor_realop_(w, t, op, b, precision=2))
    msg = refused(lambda: eu.expv_taylor_realop_(w, t, op, b, max_matvecs=need - 1))
    assert "alpha" in msg and "m* = %d" % info["m"] in msg and "s = %d" % info["s"] in msg, msg
    assert np.array_equal(eu.expv_taylor_realop(t, op, b, max_matvecs=need), eu.expv_taylor_realop(t, op, b))
    # through the raw C call: a real b in w's place, a real b inside w, a b_dtype of another precision, an unknown loc
    lib, L = eu.api.L.load(), eu.api.L
    ctx = op.ctx

    def raw(bptr, b_dtype, b_loc=L.HOST):
        eu.api._check(lib.expv_mi_expv_taylor_realop(ctx._h, op._h, t.real, t.imag, bptr, b_loc, b_dtype, w.ctypes.data, L.HOST, 0, 0, 0.0, None, None), ctx._h)
    msg = refused(lambda: raw(w.ctypes.data, L.F64))
    assert "real b" in msg, msg
    refused(lambda: raw(w.ctypes.data + 8 * n, L.F64))
    refused(lambda: raw(b.ctypes.data, L.C32))
    refused(lambda: raw(b.ctypes.data, L.C64, b_loc=7))
    raw(b.ctypes.data, L.C64)      # (and the same call with a complex b goes through)
    assert np.array_equal(w, eu.expv_taylor_realop(t, op, b))


def test_expv_taylor_still_refuses_a_complex_t_on_a_real_operator(eu):
    A, b = tc.penta(65, np.float64), tc.vector(65, np.float64)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor(1j, eu.MIOperator(A), b)
    assert ei.value.kind == "ArgumentError" and "complex t" in str(ei.value)
