"""exp(tA)b by the truncated Taylor series on the device (expv_mi_expv_taylor, eu.expv_taylor).

Truth for values: scipy.linalg.expm(tA) b in fp64 / complex128 (n <= 1000).  Bar: the device's error <= 8 x max(error of the numpy
restatement run in the operator's element type on the same input, eps_T), both relative in the max norm -- the device differs from
the restatement only in the summation order inside a row and in FMA contraction, over up to s m* ~ 1e2 .. 1e3 such roundings.
Every case's figures (restatement, device, scipy's expm_multiply for the 64-bit types) go to profiles/expv_taylor_parity.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests import expv_taylor_cases as tc
from tests._util import C2_OFFSETS, C2_VALS, banded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8.0
SMALL_N = (1, 5, 63, 64, 65, 127, 128, 129, 257)
_lines, _truths = [], {}


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
    if not _lines:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "expv_taylor_parity.txt"), "w") as f:
            f.write("# expv_taylor against scipy.linalg.expm(tA) b (n = 70001: against scipy's expm_multiply): relative max-norm errors; bar = 8 x max(restatement, eps)\n")
            f.write("%-44s %-10s %4s %8s %3s %4s %6s %5s %10s %10s %10s\n" % ("case", "dtype", "prec", "alpha", "m*", "s", "apps", "path", "restated", "device",
                                                                               "expm_mult"))
            f.write("\n".join(_lines) + "\n")
    except OSError:
        pass


def as_dense(A, W):
    return (A.toarray() if sp.issparse(A) else np.asarray(A)).astype(W)


def truth_of(key, A, b, t):
    if key not in _truths:
        W = tc.wide(A.dtype)
        _truths[key] = sl.expm(t * as_dense(A, W)) @ b.astype(W)
    return _truths[key]


def expected_path(eu, A):
    if not sp.issparse(A):
        return 2
    pi = eu.host_pattern_info(A, A.dtype)
    return 1 if pi["sell"] and pi["sell_cut"] == 0 else 2


def check(eu, tables, name, A, b, t, precision=0, op=None, path=None, opnorm=None, truth=None, truth_bar=None, key=None):
    """one call of the device against the restatement and the truth, with every assertion of the issue; returns (w, info)"""
    T = np.dtype(A.dtype)
    tab = tc.table_of(T, precision)
    mu, alpha, longest = tc.shift_norm(A, t)
    if opnorm is not None:      # matrix-free: no shift, the caller's bound
        mu, alpha = 0.0, abs(t) * opnorm
    Fr, ir = tc.restated(t, A, b, T, alpha, tables[tab], tc.TOL[tab], mu)
    if truth is None:
        truth = truth_of(key or (name, T.name, A.shape[0], complex(t)), A, b, t)
    w, info = eu.expv_taylor(t, A if op is None else op, b, precision=precision, opnorm=opnorm, return_info=True)
    w = np.asarray(w)
    assert w.dtype == T and w.shape == b.shape
    e_rest, e_dev = tc.relmax(Fr, truth), tc.relmax(w, truth)
    e_spm = float("nan")
    if T.itemsize >= (16 if T.kind == "c" else 8) and truth_bar is None and A.shape[0] > 0:
        e_spm = tc.relmax(spl.expm_multiply(t * sp.csr_matrix(A), b), truth)
    _lines.append("%-44s %-10s %4d %8.3f %3d %4d %6d %5d %10.2e %10.2e %10.2e" % (name + " n=%d" % A.shape[0] + (" ct" if isinstance(t, complex) else ""), T.name,
                                                                            precision, info["alpha"], info["m"], info["s"], info["applications"],
                                                                            info["path"], e_rest, e_dev, e_spm))
    print("[taylor]", _lines[-1])
    # norm and parameters
    assert abs(info["alpha"] - alpha) <= 4 * longest * tc.eps_of(np.float64) * alpha, (info["alpha"], alpha)
    assert (info["m"], info["s"]) == eu.host_taylor_params(info["alpha"], tab)
    assert (info["m"], info["s"]) == (ir["m"], ir["s"])
    # the stopping rule: at most one borderline stop per stage away from the restatement; never a blocking read per term
    assert abs(info["applications"] - ir["applications"]) <= info["s"], (info, ir)
    assert info["launches"] == info["m"] * info["s"] and info["host_reads"] <= 2, info
    if ir["early_stages"] > 0:
        assert info["applications"] < info["launches"], (info, ir)
    assert info["nonfinite_stage"] == 0
    assert info["path"] == (expected_path(eu, A) if path is None else path), info
    # values
    if T.itemsize >= (16 if T.kind == "c" else 8) and precision == 0 and truth_bar is None:
        assert e_rest <= 64 * tc.eps_of(T), "the 64-bit cases are chosen so that the restatement stays below 64 eps: %.2e" % e_rest
    bar = BAR * max(e_rest if truth_bar is None else truth_bar, tc.eps_of(T))
    assert e_dev <= bar, "%s: device %.3e > %g x max(restatement %.3e, eps)" % (name, e_dev, BAR, e_rest if truth_bar is None else truth_bar)
    return w, info


def alpha_for(mk, T):
    # the Schroedinger case loses digits through the hump of the series (about eps e^(alpha / s)): alpha = 10 gives s = 2 and keeps its
    # 64-bit restatement below 64 eps (17 .. 27 eps at n = 129 .. 1000; alpha = 9 is ONE stage and 1000 eps, alpha = 12: 67 eps)
    return 10.0 if (mk is tc.laplacian and np.dtype(T).kind == "c") else 40.0


def t_variants(T):
    return (False, True) if np.dtype(T).kind == "c" else (False,)


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.random8], ids=["tridiagonal", "random8"])
def test_slice_boundaries(eu, tables, mk, T, n):
    A, b = mk(n, T), tc.vector(n, T)
    for ct in t_variants(T):
        check(eu, tables, mk.__name__, A, b, tc.t_for(A, alpha_for(mk, T), ct))


@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.penta, tc.random8, tc.powerlaw, tc.dense], ids=["tridiagonal", "pentadiagonal", "random8", "powerlaw", "dense"])
def test_n1000_every_operator_form(eu, tables, mk, T):
    n = 1000
    A, b = mk(n, T), tc.vector(n, T)
    want = {tc.laplacian: 1, tc.penta: 1, tc.random8: 1, tc.powerlaw: 2, tc.dense: 2}[mk]
    for ct in t_variants(T) if mk in (tc.laplacian, tc.random8) else (False,):
        t = tc.t_for(A, alpha_for(mk, T), ct)
        for precision in (0, 1) if np.dtype(T).itemsize >= (16 if np.dtype(T).kind == "c" else 8) else (0,):
            check(eu, tables, mk.__name__, A, b, t, precision=precision, path=want)


def test_compiled_callback_with_opnorm(eu, tables):
    n = 1000
    lib = os.path.join(ROOT, "tests", "c_harness", "libstencil_cb.so")
    if not os.path.exists(lib):
        from exponentialutilities_jl_amd import build
        build.build_callback_example(verbose=False)
    cbl = C.CDLL(lib)

    class StencilOp(C.Structure):
        _fields_ = [("n", C.c_int64), ("ndiag", C.c_int), ("off", C.c_int * 8), ("coef", C.c_double * 8)]
    cbl.stencil_matvec.argtypes = [C.c_void_p] * 4
    cbl.stencil_matvec.restype = C.c_int
    assert cbl.stencil_op_sizeof() == C.sizeof(StencilOp)
    sop = StencilOp(n, len(C2_OFFSETS), (C.c_int * 8)(*C2_OFFSETS), (C.c_double * 8)(*C2_VALS))
    A = banded(n, C2_OFFSETS, C2_VALS)
    b = tc.vector(n, np.float64)
    op = eu.MIOperator(None, eu.default_context(), matvec_c=(cbl.stencil_matvec, C.addressof(sop)), shape=(n, n), dtype=np.float64, ishermitian=False)
    opnorm = float(abs(A).sum(axis=1).max())
    check(eu, tables, "callback", A, b, 20.0 / opnorm, op=op, path=2, opnorm=opnorm)
    with pytest.raises(eu.ExpvMIError) as ei:      # a callback without its bound
        eu.expv_taylor(0.1, op, b)
    assert ei.value.kind == "ArgumentError" and "opnorm" in str(ei.value)
    del sop


@pytest.mark.parametrize("T", tc.DTYPES)
def test_reordered_operator_answers_in_the_callers_ordering(eu, tables, T):
    n = 1000
    ctx = eu.Context()
    ctx.set_option("reorder", 2)      # always keep the bandwidth-reducing ordering (at this size the natural one has a single-pass form too)
    A, _ = tc.shuffled_band(n, T)
    A.sort_indices()
    b = tc.vector(n, T)
    op = eu.MIOperator(A, ctx)
    ri = op.reorder_info
    assert ri["reordered"] and ri["bandwidth_after"] < ri["bandwidth_before"], ri
    check(eu, tables, "shuffled band", A, b, tc.t_for(A, 40.0), op=op, path=1)


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_device_born_operator_with_aliased_torch_vectors(eu, torch, tables, T):
    n = 257
    A, b = tc.random8(n, T), tc.vector(n, T)
    t = tc.t_for(A, 40.0)
    At = torch.sparse_csr_tensor(torch.as_tensor(A.indptr.astype(np.int64)).cuda(), torch.as_tensor(A.indices.astype(np.int64)).cuda(),
                                 torch.as_tensor(A.data).cuda(), size=(n, n))
    op = eu.MIOperator(At)
    w_ref, info_ref = check(eu, tables, "device CSR", A, b, t, op=op, path=1)
    x = torch.as_tensor(b).cuda()
    out = eu.expv_taylor_(x, t, op, x)      # b and w are the same device tensor
    assert out is x
    assert np.array_equal(x.cpu().numpy(), w_ref), "aliased device vectors: other bits than with separate ones"
    assert eu.expv_taylor.last_info == info_ref


def test_torch_vectors_in_host_memory(eu, torch):
    n = 129
    A, b = tc.penta(n, np.float64), tc.vector(n, np.float64)
    t = tc.t_for(A, 20.0)
    want = eu.expv_taylor(t, A, b)
    bt = torch.as_tensor(b.copy())
    w = eu.expv_taylor(t, A, bt)
    assert torch.is_tensor(w) and not w.is_cuda and np.array_equal(w.numpy(), want)
    assert eu.expv_taylor_(bt, t, A, bt) is bt and np.array_equal(bt.numpy(), want)


@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_more_workgroups_than_compute_units(eu, tables, T):
    """n = 70 001: the ticket's last arrival is not the last workgroup launched.  Values against scipy's expm_multiply on the CPU; bar
    from its own agreement with the restatement."""
    n = 70001
    A, b = tc.laplacian(n, T), tc.vector(n, T)
    t = tc.t_for(A, 10.0)
    ref = spl.expm_multiply(t * A, b)
    mu, alpha, _ = tc.shift_norm(A, t)
    Fr = tc.restated(t, A, b, T, alpha, tables[0], tc.TOL[0], mu)[0]
    check(eu, tables, "laplacian", A, b, t, path=1, truth=ref, truth_bar=tc.relmax(Fr, ref))


def test_long_series_reads_the_device_twice(eu, tables):
    """Laplacian, t = 40: alpha = 80, s m* ~ 450 launches, two blocking reads"""
    n = 1000
    A, b = tc.laplacian(n, np.float64), tc.vector(n, np.float64)
    _, info = check(eu, tables, "laplacian t=40", A, b, 40.0, path=1)
    assert info["launches"] >= 400 and info["host_reads"] == 2 and info["early_stages"] == info["s"], info


@pytest.mark.parametrize("mk,path", [(tc.random8, 1), (tc.laplacian, 1), (tc.powerlaw, 2), (tc.dense, 2)], ids=["sell", "dia", "overflow", "dense"])
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_two_calls_give_the_same_bits(eu, mk, path, T):
    n = 1000
    A, b = mk(n, T), tc.vector(n, T)
    op = eu.MIOperator(A)
    t = tc.t_for(A, 30.0)
    w1, i1 = eu.expv_taylor(t, op, b, return_info=True)
    w2, i2 = eu.expv_taylor(t, op, b, return_info=True)
    assert i1["path"] == path and i1 == i2
    assert np.array_equal(np.asarray(w1).view(np.uint8), np.asarray(w2).view(np.uint8))


# ---- edge cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES)
def test_t_zero_returns_b_bit_for_bit(eu, T):
    n = 129
    A, b = tc.random8(n, T), tc.vector(n, T)
    w, info = eu.expv_taylor(0.0, A, b, return_info=True)
    assert np.array_equal(np.asarray(w).view(np.uint8), b.view(np.uint8))
    assert (info["m"], info["s"], info["applications"], info["launches"], info["alpha"]) == (0, 1, 0, 0, 0.0)


@pytest.mark.parametrize("T", tc.DTYPES)
def test_zero_vector_costs_no_application(eu, T):
    n = 257
    A = tc.random8(n, T)
    w, info = eu.expv_taylor(tc.t_for(A, 40.0), A, np.zeros(n, dtype=T), return_info=True)
    assert not np.any(np.asarray(w)) and info["applications"] == 0 and info["launches"] == info["m"] * info["s"] > 0
    assert info["normF"] == 0.0 and info["nonfinite_stage"] == 0


@pytest.mark.parametrize("T", tc.DTYPES)
def test_shift_annihilates_a_multiple_of_the_identity(eu, T):
    n, t = 129, 0.75
    c = np.dtype(T).type(1.5 - 0.5j) if np.dtype(T).kind == "c" else np.dtype(T).type(1.5)
    A = (sp.identity(n, format="csr") * c).astype(T)
    b = tc.vector(n, T)
    w, info = eu.expv_taylor(t, A, b, return_info=True)
    assert info["alpha"] == 0.0 and (info["m"], info["s"], info["applications"]) == (0, 1, 0)
    W = tc.wide(T)
    want = np.exp(W(t) * W(c)) * b.astype(W)
    # 2 ulp: the rounding of the factor to T (eps / 2) and one product (real: eps / 2; complex: sqrt(5) eps / 2 in modulus)
    assert np.max(np.abs(np.asarray(w).astype(W) - want) / np.abs(want)) <= 2 * tc.eps_of(T)
    mu = info["mu"]
    assert abs(mu - complex(c) if np.dtype(T).kind == "c" else mu - float(c)) <= 4 * tc.eps_of(np.float64) * abs(c)


def test_empty_operator_does_nothing(eu):
    h = C.c_void_p()
    ctx = eu.default_context()
    lib = eu.api.L.load()
    rp = np.zeros(1, dtype=np.int32)
    eu.api._check(lib.expv_mi_op_create_csr(ctx._h, eu.api.L.F64, 0, rp.ctypes.data, None, None, 4, 0, C.byref(h)), ctx._h)
    try:
        info, dinfo = (C.c_int64 * 8)(*([7] * 8)), (C.c_double * 4)(*([7.0] * 4))
        eu.api._check(lib.expv_mi_expv_taylor(ctx._h, h, 1.0, 0.0, None, 0, None, 0, 0, 0, 0.0, info, dinfo), ctx._h)
        assert list(info) == [0] * 8 and list(dinfo) == [0.0] * 4
    finally:
        lib.expv_mi_op_destroy(h)


def test_max_matvecs_at_and_below_the_need(eu):
    n = 257
    A, b = tc.penta(n, np.float64), tc.vector(n, np.float64)
    t = tc.t_for(A, 40.0)
    op = eu.MIOperator(A)
    _, info = eu.expv_taylor(t, op, b, return_info=True)
    need = info["m"] * info["s"]
    w = np.full(n, 7.0)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_(w, t, op, b, max_matvecs=need - 1)
    msg = str(ei.value)
    assert ei.value.kind == "ArgumentError" and "alpha" in msg and "m* = %d" % info["m"] in msg and "s = %d" % info["s"] in msg, msg
    assert np.all(w == 7.0), "a refused call must leave w alone"
    w2 = eu.expv_taylor(t, op, b, max_matvecs=need)
    assert np.array_equal(w2, eu.expv_taylor(t, op, b))


def test_real_operator_refuses_a_complex_t(eu):
    A, b = tc.penta(65, np.float64), tc.vector(65, np.float64)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor(0.5 + 0.25j, A, b)
    assert ei.value.kind == "ArgumentError"
    for bad in (2, -1):
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.expv_taylor(0.5, A, b, precision=bad)
        assert ei.value.kind == "ArgumentError"


@pytest.mark.parametrize("mk", [tc.random8, tc.powerlaw], ids=["fused", "update"])
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_an_infinite_entry_is_returned_not_raised(eu, tables, mk, T):
    n = 257
    A, b = mk(n, T), tc.vector(n, T)
    t = tc.t_for(A, 40.0)
    op = eu.MIOperator(A)
    bad = b.copy()
    bad[n // 3] = np.inf
    w, info = eu.expv_taylor(t, op, bad, return_info=True)
    assert info["nonfinite_stage"] >= 1 and not np.all(np.isfinite(np.asarray(w))) and not np.isfinite(info["normF"])
    assert info["applications"] < info["launches"] or info["s"] == 1
    check(eu, tables, mk.__name__ + " after inf", A, b, t, op=op)      # the context and the operator are as good as before
