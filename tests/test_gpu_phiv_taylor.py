"""w = sum_k t^k phi_k(tA) u_k by the truncated Taylor series on the device (expv_mi_phiv_taylor, eu.phiv_taylor).

Truth: the first n rows of scipy.linalg.expm(t [A W; 0 J]) [u_0; e_p] in fp64 / complex128 (tests/phiv_taylor_cases.py).  Bar: the
device's error <= 8 x max(error of the numpy restatement run in the operator's element type on the same input, eps_T), both relative
in the max norm -- as in tests/test_gpu_expv_taylor.py, the device differs from the restatement only in the summation order inside a
row and in FMA contraction.  Every case's figures go to profiles/phiv_taylor_parity.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import expv_taylor_cases as tc
from tests import phiv_taylor_cases as pc
from tests._util import C2_OFFSETS, C2_VALS, banded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8.0
_lines, _cache = [], {}


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
        with open(os.path.join(ROOT, "profiles", "phiv_taylor_parity.txt"), "w") as f:
            f.write("# phiv_taylor against the first n rows of scipy.linalg.expm(t [A W; 0 J]) [u_0; e_p]: relative max-norm errors; bar = 8 x max(restatement, eps)\n")
            f.write("%-40s %-10s %2s %8s %3s %4s %6s %5s %9s %9s %10s %10s\n" % ("case", "dtype", "p", "alpha", "m*", "s", "apps", "path", "nu", "U", "restated",
                                                                               "device"))
            f.write("\n".join(_lines) + "\n")
    except OSError:
        pass


def expected_path(eu, A):
    if not sp.issparse(A):
        return 2
    pi = eu.host_pattern_info(A, A.dtype)
    return 1 if pi["sell"] and pi["sell_cut"] == 0 else 2


def reference(key, tables, t, A, B, opnorm=None, truth_A=None):
    """(restatement, its info, truth) of a case, computed once"""
    if key not in _cache:
        T = np.dtype(B.dtype)
        tab = tc.table_of(T, 0)
        Fr, ir = pc.restated(t, A, B, T, tables[tab], tc.TOL[tab], opnorm=opnorm)
        _cache[key] = (Fr, ir, pc.truth(t, A if truth_A is None else truth_A, B))
    return _cache[key]


def check(eu, tables, name, A, B, t, op=None, path=None, opnorm=None, key=None):
    """one call of the device against the restatement and the truth, with every assertion of the parity test; returns (w, info)"""
    T = np.dtype(B.dtype)
    n, p = B.shape[0], B.shape[1] - 1
    tab = tc.table_of(T, 0)
    Fr, ir, truth = reference(key or (name, T.name, n, p, complex(t)), tables, t, A, B, opnorm)
    w, info = eu.phiv_taylor(t, A if op is None else op, B, opnorm=opnorm, return_info=True)
    w = np.asarray(w)
    assert w.dtype == T and w.shape == (n,)
    e_rest, e_dev = tc.relmax(Fr, truth), tc.relmax(w, truth)
    _lines.append("%-40s %-10s %2d %8.3f %3d %4d %6d %5d %9.3g %9.3g %10.2e %10.2e" % (name + " n=%d" % n + (" ct" if isinstance(t, complex) else ""), T.name, p,
                                                                                   info["alpha"], info["m"], info["s"], info["applications"], info["path"],
                                                                                   info["nu"], info["U"], e_rest, e_dev))
    print("[phiv_taylor]", _lines[-1])
    # norm and parameters
    assert abs(info["alpha"] - ir["alpha"]) <= 4 * (ir["longest"] + p) * tc.eps_of(np.float64) * ir["alpha"], (info["alpha"], ir["alpha"])
    assert info["nu"] == ir["nu"] and info["U"] == ir["U"], (info, ir)
    assert (info["m"], info["s"]) == eu.host_taylor_params(info["alpha"], tab)
    assert (info["m"], info["s"]) == (ir["m"], ir["s"])
    # the stopping rule: at most one borderline stop per stage away from the restatement; never a blocking read per term
    assert abs(info["applications"] - ir["applications"]) <= info["s"], (info, ir)
    assert info["launches"] == info["m"] * info["s"] and info["host_reads"] <= 3, info
    assert info["nonfinite_stage"] == 0
    assert info["path"] == (expected_path(eu, A) if path is None else path), info
    # values
    bar = BAR * max(e_rest, tc.eps_of(T))
    assert e_dev <= bar, "%s p=%d: device %.3e > %g x max(restatement %.3e, eps)" % (name, p, e_dev, BAR, e_rest)
    return w, info


def bits(x):
    return np.ascontiguousarray(np.asarray(x)).view(np.uint8)


# ---- parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.SMALL_N)
@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("kind", pc.OPERATORS)
def test_parity(eu, tables, kind, T, n):
    A = pc.operator(kind, n, T)
    op = eu.MIOperator(A)
    for n_, p, only_last, ct in pc.parity_cases(T):
        if n_ != n or only_last:
            continue
        B = pc.block(n, p, T)
        check(eu, tables, kind, A, B, pc.t_for(A, B, pc.alpha_for(kind, T), ct), op=op)


@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("kind", pc.OPERATORS)
def test_only_the_last_column_is_not_zero(eu, tables, kind, T):
    """u_0 .. u_{p-1} = 0: the first terms of the first stage are zero, and only the floor under the stopping test keeps it going"""
    for n, p, only_last, ct in pc.parity_cases(T):
        if not only_last:
            continue
        A = pc.operator(kind, n, T)
        B = pc.block(n, p, T, only_last=True)
        w, info = check(eu, tables, kind + " only u_p", A, B, pc.t_for(A, B, pc.alpha_for(kind, T), ct))
        assert np.any(w != 0) and info["applications"] >= p


# ---- p = 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (65, 257))
@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("kind", pc.OPERATORS)
def test_one_column_is_expv_taylor_bit_for_bit(eu, kind, T, n):
    A, b = pc.operator(kind, n, T), tc.vector(n, T)
    op = eu.MIOperator(A)
    t = tc.t_for(A, pc.alpha_for(kind, T))
    want, iw = eu.expv_taylor(t, op, b, return_info=True)
    w, info = eu.phiv_taylor(t, op, b[:, None], return_info=True)
    assert np.array_equal(bits(w), bits(want))
    assert {k: info[k] for k in iw} == iw and info["nu"] == 1.0 and info["U"] == 0.0


# ---- exact scaling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("kind", pc.OPERATORS)
def test_scaling_B_by_a_power_of_two_scales_w_exactly(eu, kind, T):
    n, p = 129, 3
    A, B = pc.operator(kind, n, T), pc.block(n, p, T)
    op = eu.MIOperator(A)
    t = pc.t_for(A, B, pc.alpha_for(kind, T))
    w1, i1 = eu.phiv_taylor(t, op, B, return_info=True)
    sc = np.dtype(T).type(2.0 ** -40)
    w2, i2 = eu.phiv_taylor(t, op, np.asfortranarray(B * sc), return_info=True)
    assert np.array_equal(bits(np.asarray(w1) * sc), bits(w2))
    assert i2["nu"] == i1["nu"] * 2.0 ** 40 and i2["U"] == i1["U"] * 2.0 ** -40 and i2["alpha"] == i1["alpha"]
    assert (i2["m"], i2["s"], i2["applications"]) == (i1["m"], i1["s"], i1["applications"])


# ---- a matrix-free operator: mu = 0, the coefficients of every term j > p are zero ----------------------------------------------
def test_matrix_free_operator_skips_B_after_p_terms(eu, torch, tables):
    n, p = 1000, 3
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
    op = eu.MIOperator(None, eu.default_context(), matvec_c=(cbl.stencil_matvec, C.addressof(sop)), shape=(n, n), dtype=np.float64, ishermitian=False)
    opnorm = float(abs(A).sum(axis=1).max())
    B = pc.block(n, p, np.float64)
    t = 20.0 / opnorm
    # a host-built device block, followed by a guard region that no launch may change
    guard = 4096
    buf = torch.full((n * (p + 1) + guard,), -7.0, dtype=torch.float64, device="cuda")
    buf[: n * (p + 1)] = torch.as_tensor(np.ascontiguousarray(B.T).ravel()).cuda()
    Bt = buf[: n * (p + 1)].view(p + 1, n).t()      # column-major n x (p + 1)
    Fr, ir, truth = reference(("callback", n, p), tables, t, A, B, opnorm=opnorm)
    w, info = eu.phiv_taylor(t, op, Bt, opnorm=opnorm, return_info=True)
    w = w.cpu().numpy()
    assert ir["skipped"] == ir["s"] * (ir["m"] - p) > 0, "mu = 0: J is nilpotent, every term j > p has zero coefficients"
    assert info["mu"] == 0.0 and info["path"] == 2
    assert (info["m"], info["s"], info["launches"]) == (ir["m"], ir["s"], ir["m"] * ir["s"])
    assert abs(info["applications"] - ir["applications"]) <= info["s"]
    e_rest, e_dev = tc.relmax(Fr, truth), tc.relmax(w, truth)
    _lines.append("%-40s %-10s %2d %8.3f %3d %4d %6d %5d %9.3g %9.3g %10.2e %10.2e" % ("callback n=%d" % n, "float64", p, info["alpha"], info["m"], info["s"],
                                                                                   info["applications"], info["path"], info["nu"], info["U"], e_rest, e_dev))
    assert e_dev <= BAR * max(e_rest, tc.eps_of(np.float64))
    assert bool((buf[n * (p + 1):] == -7.0).all()) and np.array_equal(Bt.cpu().numpy(), B)
    del sop


# ---- layouts and locations -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("kind", ["tridiagonal", "dense"])
def test_layouts_and_locations_give_the_same_bits(eu, torch, kind, T):
    n, p = 129, 3
    A, B = pc.operator(kind, n, T), pc.block(n, p, T)
    op = eu.MIOperator(A)
    t = pc.t_for(A, B, pc.alpha_for(kind, T))
    want = bits(eu.phiv_taylor(t, op, B))
    wide_f = np.zeros((n + 5, p + 1), dtype=T, order="F")      # column-major, ldb = n + 5
    wide_f[:n] = B
    wide_c = np.zeros((n, p + 4), dtype=T, order="C")          # row-major, ldb = p + 4
    wide_c[:, : p + 1] = B
    for name, Bx in (("host row-major", np.ascontiguousarray(B)), ("host column-major ld", wide_f[:n]), ("host row-major ld", wide_c[:, : p + 1])):
        assert np.array_equal(bits(eu.phiv_taylor(t, op, Bx)), want), name
    for name, Bx in (("device row-major", torch.as_tensor(np.ascontiguousarray(B)).cuda()),
                     ("device column-major", torch.as_tensor(np.ascontiguousarray(B.T)).cuda().t()),
                     ("device column-major ld", torch.as_tensor(np.ascontiguousarray(wide_f.T)).cuda().t()[:n]),
                     ("device row-major ld", torch.as_tensor(wide_c).cuda()[:, : p + 1])):
        w = eu.phiv_taylor(t, op, Bx)
        assert torch.is_tensor(w) and w.is_cuda and np.array_equal(bits(w.cpu().numpy()), want), name
    # w is column 0 of B, on the host and on the device
    Bh = B.copy(order="F")
    assert eu.phiv_taylor_(Bh[:, 0], t, op, Bh) is not None
    assert np.array_equal(bits(Bh[:, 0]), want) and np.array_equal(Bh[:, 1:], B[:, 1:])
    Bd = torch.as_tensor(np.ascontiguousarray(B.T)).cuda().t()
    eu.phiv_taylor_(Bd[:, 0], t, op, Bd)
    got = Bd.cpu().numpy()
    assert np.array_equal(bits(got[:, 0]), want) and np.array_equal(got[:, 1:], B[:, 1:])


# ---- a reordered operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.DTYPES)
def test_reordered_operator_answers_in_the_callers_ordering(eu, tables, T):
    n, p = 257, 3
    ctx = eu.Context()
    ctx.set_option("reorder", 2)      # always keep the bandwidth-reducing ordering
    A, _ = tc.shuffled_band(n, T)
    A.sort_indices()
    B = pc.block(n, p, T)
    op = eu.MIOperator(A, ctx)
    assert op.reorder_info["reordered"], op.reorder_info
    check(eu, tables, "shuffled band", A, B, pc.t_for(A, B, 40.0), op=op, path=1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_w_untouched(eu, torch):
    n, p = 65, 3
    A, B = tc.penta(n, np.float64), pc.block(n, p, np.float64)
    op = eu.MIOperator(A)
    t = pc.t_for(A, B, 40.0)
    lib = eu.api.L.load()
    w = np.full(n, 7.0)
    info, dinfo = (C.c_int64 * 8)(), (C.c_double * 8)()

    def raw(ncols, w_ptr=None):
        return lib.expv_mi_phiv_taylor(op.ctx._h, op._h, t, 0.0, B.ctypes.data, n, ncols, 0, 0, w.ctypes.data if w_ptr is None else w_ptr, 0, 0, 0, 0.0,
                                       info, dinfo)
    for ncols in (0, 10):
        assert raw(ncols) == 2 and "ncols = %d" % ncols in lib.expv_mi_last_error(op.ctx._h).decode()
    assert np.all(w == 7.0)
    with pytest.raises(eu.ExpvMIError) as ei:      # ten columns through the front end
        eu.phiv_taylor_(w, t, op, np.zeros((n, 10)))
    assert ei.value.kind == "ArgumentError" and np.all(w == 7.0)
    before = B.copy()
    assert raw(p + 1, B[:, 1].ctypes.data) == 2      # w is column 1
    assert "overlaps a column of B other than column 0" in lib.expv_mi_last_error(op.ctx._h).decode()
    assert raw(p + 1, B.ctypes.data + 8 * (n - 1)) == 2      # w starts in column 0 and runs into column 1
    assert np.array_equal(B, before)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.phiv_taylor_(w, 0.5 + 0.25j, op, B)
    assert ei.value.kind == "ArgumentError" and "complex t" in str(ei.value) and np.all(w == 7.0)
    _, i0 = eu.phiv_taylor(t, op, B, return_info=True)
    need = i0["m"] * i0["s"]
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.phiv_taylor_(w, t, op, B, max_matvecs=need - 1)
    msg = str(ei.value)
    assert ei.value.kind == "ArgumentError" and "m* = %d" % i0["m"] in msg and "s = %d" % i0["s"] in msg and np.all(w == 7.0)
    assert np.array_equal(eu.phiv_taylor_(w, t, op, B, max_matvecs=need), eu.phiv_taylor(t, op, B))
    wd = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")      # a refused call with a device w
    with pytest.raises(eu.ExpvMIError):
        eu.phiv_taylor_(wd, t, op, B, max_matvecs=1)
    assert bool((wd == 7.0).all())
