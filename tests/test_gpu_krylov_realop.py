"""Mixed calls on the device: a real operator (Float64 / Float32) with vectors and a subspace of its complex type, the operator
read as it is stored (expv_mi_op_apply_complex, expv_mi_arnoldi / _lanczos with a complex dtype_T, expv_mi_expv_realop,
expv_mi_phiv_timestep_realop; ``keep_real=True`` in Python).

Bars (the project's own): device vs oracle at the same m 1e-12 on H (relative to its largest entry), V (max abs) and w (relative) --
the TOL of tests/test_gpu_parity.py; 1e-10 against scipy.linalg.expm(tA) b in the converged regime; 3e-5 for the 32-bit types; mul!
per real component |y - A x| <= (k + 2) u (|A| |x|), derived in tests/krylov_realop_cases.py.  The oracle is the yardstick as it
stands: tests/test_krylov_realop_cpu.py pins that it gives a real matrix under a complex b what its complex cast gives."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from oracle import krylov_oracle as ko
from tests import krylov_realop_cases as kc
from tests._util import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_TRUTH, TOL32 = kc.TOL, kc.TOL_TRUTH, kc.TOL32
TWO_KERNEL, MODULAR = {"two_kernel"}, {"modular"}


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def form_of(op):
    """the step form of the factorisation that just ran on the operator's context: (set of path names, real_operator)"""
    st = op.ctx.last_path()
    return set(st["path"]), st["real_operator"]


def expv_form_of(eu, op, b, **kw):
    """the same for the private subspace of a whole-call expv with these options, from its own stats"""
    eu.expv(0.1, op, b, keep_real=True, **kw)
    st = eu.expv.last_stats
    assert (set(st["path"]), st["real_operator"]) == form_of(op)
    return set(st["path"]), st["real_operator"]


# ---- mul! -------------------------------------------------------------------------------------------------------------------------
def check_mul(eu, torch, op, A, R, where, applies):
    """matvec_complex against the extended-precision product, per real component, and the application counter"""
    n = A.shape[0]
    Cd = kc.complex_of(R)
    x = kc.cvector(n, R, seed=21)
    re, im = kc.mul_reference(A, x)
    bre, bim = kc.mul_bound(A, x, R)
    c0 = op.ctx.counters()["op_applies"]
    if where == "device":
        y = op.matvec_complex(torch.from_numpy(x).cuda())
        assert y.is_cuda and y.dtype == (torch.complex64 if Cd == np.complex64 else torch.complex128)
        y = y.cpu().numpy()
    else:
        y = op.matvec_complex(x)
        assert isinstance(y, np.ndarray)
    assert op.ctx.counters()["op_applies"] - c0 == applies
    assert y.dtype == Cd and y.shape == (n,)
    ere, eim = np.abs(y.real.astype(np.longdouble) - re), np.abs(y.imag.astype(np.longdouble) - im)
    worst = max(float(np.max(ere / np.maximum(bre, 1e-300))), float(np.max(eim / np.maximum(bim, 1e-300))))
    print("[mul! realop] n=%d %s %s: worst |y - Ax| / bound = %.3f" % (n, np.dtype(R).name, where, worst))
    assert np.all(ere <= bre) and np.all(eim <= bim), "mul!: |y - A x| exceeds (k + 2) u |A| |x| by a factor %.3f" % worst


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("R", kc.REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("n", kc.MUL_N)
def test_mul_sell_slice_and_pack_boundaries(eu, torch, n, R, where):
    A = kc.sell5(n, R)
    check_mul(eu, torch, eu.MIOperator(A), A, R, where, applies=1)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("R", kc.REALS, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["gdia", "overflow", "dense"])
def test_mul_other_storage_forms(eu, torch, kind, R, where):
    A = {"gdia": kc.gdia, "overflow": kc.overflow, "dense": kc.dense}[kind](R=R)
    if kind == "overflow":
        info = eu.host_pattern_info(A, R)
        assert info["sell_cut"] > 0 and "overflow" in info["path"], info
    if kind == "gdia":
        assert eu.host_pattern_info(A, R)["general_dia_diagonals"] == 5
    # (one walk of the operator on a fused form; the operator's own real mul! on each plane otherwise)
    check_mul(eu, torch, eu.MIOperator(A), A, R, where, applies=1 if kind == "gdia" else 2)


@pytest.mark.parametrize("R", kc.REALS, ids=["f64", "f32"])
def test_mul_matrix_free_callback_sees_real_vectors(eu, torch, R):
    n = 300
    rng = np.random.default_rng(31)
    d, lo, up = (rng.standard_normal(n).astype(R), rng.standard_normal(n - 1).astype(R), rng.standard_normal(n - 1).astype(R))
    A = sp.diags([lo, d, up], (-1, 0, 1), format="csr").astype(R)
    dd, ld, ud = (torch.from_numpy(v).cuda() for v in (d, lo, up))
    seen = []

    def matvec(x):
        seen.append((x.dtype, tuple(x.shape)))
        y = dd * x
        y[1:] += ld * x[:-1]
        y[:-1] += ud * x[1:]
        return y

    op = eu.MIOperator(None, matvec=matvec, shape=(n, n), dtype=R)
    check_mul(eu, torch, op, A, R, "device", applies=2)
    rdt = torch.float32 if R == np.float32 else torch.float64
    assert seen == [(rdt, (n,)), (rdt, (n,))], seen      # the real and the imaginary plane, as real n-vectors


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("R", kc.REALS, ids=["f64", "f32"])
def test_mul_reordered_operator(eu, torch, R, where):
    ctx = eu.Context()
    ctx.set_option("reorder", 2)      # always keep the bandwidth-reducing ordering
    A = kc.permuted_band(R=R)
    op = eu.MIOperator(A, ctx)
    ri = op.reorder_info
    assert ri["reordered"] and ri["bandwidth_after"] < ri["bandwidth_before"], ri
    check_mul(eu, torch, op, A, R, where, applies=1)


def test_mul_refuses_a_complex_operator(eu):
    op = eu.MIOperator(kc.sell5(129).astype(np.complex128))
    with pytest.raises(eu.ExpvMIError, match="op_apply_complex") as ei:
        op.matvec_complex(kc.cvector(129))
    assert ei.value.kind == "ArgumentError"


# ---- arnoldi! against the oracle ------------------------------------------------------------------------------------------------------
def arnoldi_pair(eu, op, A, b, m, iop=0, ortho="auto", herm=False, **kw):
    n = A.shape[0]
    Ks = eu.KrylovSubspace(np.complex128, np.float64 if herm else np.complex128, n, m, ctx=op.ctx)
    eu.arnoldi_(Ks, op, b, m=m, iop=iop, ishermitian=herm, ortho=ortho, keep_real=True, **kw)
    Ko = ko.KrylovSubspace(complex, float if herm else complex, n, m)
    ko.arnoldi_(Ko, A, b, m=m, iop=iop, ishermitian=herm)
    return Ks, Ko


def assert_parity(Ks, Ko, what):
    assert Ks.m == Ko.m and Ks.wasbreakdown == Ko.wasbreakdown
    assert abs(Ks.beta - Ko.beta) <= 1e-14 * Ko.beta
    close(Ks.getH(), Ko.getH(), TOL, "realop %s H" % what, mat=True)
    close(Ks.getV(), Ko.getV(), TOL, "realop %s V (max abs)" % what, absolute=True)


@pytest.fixture(scope="module")
def natural(eu):
    """a context that stores operators in the caller's ordering: the scattered band stays on SELL slots with far columns"""
    ctx = eu.Context()
    ctx.set_option("reorder", 0)
    ctx.set_option("patch", 0)
    return ctx


@pytest.mark.parametrize("ortho", ["mgs", "lowsync"])
@pytest.mark.parametrize("n,m,iop", kc.ARNOLDI_SHAPES)
def test_arnoldi_parity_and_step_form(eu, natural, n, m, iop, ortho):
    A, b = kc.scattered_band(n), kc.cvector(n)
    op = eu.MIOperator(A, natural)
    assert op.dtype == np.float64 and not op.reorder_info["reordered"]
    want = (TWO_KERNEL if ortho == "lowsync" else MODULAR, True)
    Ks, Ko = arnoldi_pair(eu, op, A, b, m, iop, ortho)
    assert form_of(op) == want          # of the factorisation whose H and V are compared below
    assert Ks.T == np.complex128
    assert_parity(Ks, Ko, "arnoldi n=%d m=%d iop=%d %s" % (n, m, iop, ortho))
    assert expv_form_of(eu, op, b, m=m, iop=iop, ortho=ortho, ishermitian=False) == want


def test_arnoldi_reordered_operator(eu):
    """the default context may store the scattered band in a bandwidth-reducing ordering: the mixed call keeps it, and V comes
    back in the caller's ordering"""
    n, m = 2001, 17
    ctx = eu.Context()
    ctx.set_option("reorder", 2)
    A, b = kc.scattered_band(n), kc.cvector(n)
    op = eu.MIOperator(A, ctx)
    assert op.reorder_info["reordered"], op.reorder_info
    Ks, Ko = arnoldi_pair(eu, op, A, b, m, 0, "lowsync")
    assert form_of(op) == (TWO_KERNEL, True)
    assert_parity(Ks, Ko, "arnoldi reordered operator")
    assert expv_form_of(eu, op, b, m=m, ortho="lowsync", ishermitian=False) == (TWO_KERNEL, True)


def test_arnoldi_general_diagonal_form(eu):
    A, b = kc.grid_band(), kc.cvector(1000)
    assert eu.host_pattern_info(A)["general_dia_diagonals"] == 5
    op = eu.MIOperator(A)
    Ks, Ko = arnoldi_pair(eu, op, A, b, 20, 0, "lowsync")
    assert form_of(op) == (TWO_KERNEL, True)
    assert_parity(Ks, Ko, "arnoldi general DIA")
    assert expv_form_of(eu, op, b, m=20, ortho="lowsync", ishermitian=False) == (TWO_KERNEL, True)


@pytest.mark.parametrize("case", ["window_over_64", "overflow_rows", "fused_off", "dense"])
def test_arnoldi_modular_forms(eu, case):
    ctx = eu.Context()
    ctx.set_option("reorder", 0)
    n, m = 300, 20
    A = kc.scattered_band(n)
    if case == "window_over_64":
        m = 66
    elif case == "overflow_rows":
        A, n = kc.scattered_band_long_row(), 600
        info = eu.host_pattern_info(A)
        assert info["sell_cut"] > 0 and "overflow" in info["path"], info
    elif case == "fused_off":
        ctx.set_option("fused", 0)
    elif case == "dense":
        A, n = kc.dense_band(), 67
    b = kc.cvector(n)
    op = eu.MIOperator(A, ctx)
    Ks, Ko = arnoldi_pair(eu, op, A, b, m, 0, "lowsync")
    assert form_of(op) == (MODULAR, True)
    assert_parity(Ks, Ko, "arnoldi %s" % case)
    assert expv_form_of(eu, op, b, m=m, ortho="lowsync", ishermitian=False) == (MODULAR, True)


def test_arnoldi_float32_operator(eu):
    n, m = 513, 20
    A, b = kc.scattered_band(n, np.float32), kc.cvector(n, np.float32)
    op = eu.MIOperator(A)
    assert op.dtype == np.float32
    Ko = ko.arnoldi(A.astype(np.float64), b.astype(np.complex128), m=m, ishermitian=False)
    for ortho in ("lowsync", "mgs"):
        Ks = eu.arnoldi(op, b, m=m, ishermitian=False, ortho=ortho, keep_real=True)
        assert Ks.T == np.complex64 and Ks.m == Ko.m
        close(Ks.getH(), Ko.getH(), TOL32, "realop arnoldi f32 H %s" % ortho, mat=True)
        close(Ks.getV(), Ko.getV(), TOL32, "realop arnoldi f32 V %s (max abs)" % ortho, absolute=True)


# ---- lanczos! -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mk,n,form", [(kc.scattered_sym, 513, TWO_KERNEL), (kc.sym5, 1000, TWO_KERNEL), (kc.sym_sell, 513, MODULAR)],
                         ids=["sell", "band", "irregular"])
def test_lanczos_real_tridiagonal_complex_basis(eu, natural, mk, n, form):
    """(irregular: the symmetrised random rows have uneven lengths -- slots up to a cut + overflow entries, so the modular launches)"""
    A, b, m = mk(n), kc.cvector(n), 20
    op = eu.MIOperator(A, natural)
    assert op.ishermitian and (eu.host_pattern_info(A)["sell_cut"] > 0) == (form == MODULAR)
    Ks = eu.arnoldi(op, b, m=m, keep_real=True)          # ishermitian=None asks the operator -> lanczos!
    Ko = ko.arnoldi(A, b, m=m)
    assert Ks.T == np.complex128 and Ks.U == np.float64 and Ks.getH().dtype == np.float64 and Ks.getV().dtype == np.complex128
    assert_parity(Ks, Ko, "lanczos (asked the operator) n=%d" % n)
    K2 = eu.KrylovSubspace(np.complex128, np.float64, n, m, ctx=natural)
    eu.lanczos_(K2, op, b, m=m, keep_real=True)
    assert form_of(op) == (form, True)
    assert_parity(K2, Ko, "lanczos! n=%d" % n)
    assert expv_form_of(eu, op, b, m=m) == (form, True)


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("herm", [False, True], ids=["arnoldi", "lanczos"])
def test_happy_breakdown(eu, herm):
    n = 200
    A = sp.diags([np.linspace(-3.0, -1.0, n)], [0], format="csr")
    b = np.zeros(n, dtype=np.complex128)
    b[[7, 90, 150]] = (1.0 + 2.0j, -0.5j, 0.25 - 1.0j)      # three eigenvectors of a diagonal operator
    Ks = eu.arnoldi(A, b, m=10, ishermitian=herm, keep_real=True)
    assert Ks.m == 3 and Ks.wasbreakdown
    w = eu.expv(-0.7j, A, b, m=10, ishermitian=herm, keep_real=True)
    assert eu.expv.last_stats["real_operator"] and eu.expv.last_stats["wasbreakdown"] and eu.expv.last_stats["m"] == 3
    close(w, np.exp(-0.7j * A.diagonal()) * b, TOL, "realop happy breakdown herm=%s" % herm)


def test_zero_starting_vector(eu):
    n = 300
    A = kc.sell5(n)
    z = np.zeros(n, dtype=np.complex128)
    Ks = eu.arnoldi(A, z, m=5, ishermitian=False, keep_real=True)
    assert Ks.beta == 0.0
    w = eu.expv(-0.7j, A, z, m=5, keep_real=True)
    assert w.dtype == np.complex128 and not np.any(w) and not np.any(np.isnan(w))


@pytest.mark.parametrize("ortho", ["lowsync", "mgs"])
def test_continuation_and_resize(eu, ortho):
    n = 513
    A, b = kc.scattered_band(n), kc.cvector(n)
    op = eu.MIOperator(A)
    Ks = eu.KrylovSubspace(np.complex128, np.complex128, n, 20)
    eu.arnoldi_(Ks, op, b, m=10, ishermitian=False, ortho=ortho, keep_real=True)
    eu.arnoldi_(Ks, op, b, m=20, init=11, ishermitian=False, ortho=ortho, keep_real=True)
    Ko = ko.KrylovSubspace(complex, complex, n, 20)
    ko.arnoldi_(Ko, A, b, m=20, ishermitian=False)
    assert_parity(Ks, Ko, "continuation init=11 %s" % ortho)
    Ks.resize(25)
    assert Ks.maxiter == 25 and Ks.m == 25 and np.all(Ks.H == 0)
    eu.arnoldi_(Ks, op, b, m=25, ishermitian=False, ortho=ortho, keep_real=True)
    Ko = ko.KrylovSubspace(complex, complex, n, 25)
    ko.arnoldi_(Ko, A, b, m=25, ishermitian=False)
    assert_parity(Ks, Ko, "after resize %s" % ortho)


def test_defer_tail_then_expv_on_the_subspace(eu):
    n, m, t = 513, 20, 0.3 - 0.4j
    A, b = kc.scattered_band(n), kc.cvector(n)
    Ks, Ko = arnoldi_pair(eu, eu.MIOperator(A), A, b, m, 0, "lowsync", defer_tail=True)
    w = eu.expv_(np.empty(n, dtype=np.complex128), t, Ks)
    close(w, ko.expv_(np.empty(n, dtype=np.complex128), t, Ko), TOL, "realop defer_tail + expv!(w, t, Ks)")
    assert_parity(Ks, Ko, "defer_tail")


# ---- expv(t, A, b, keep_real=True) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["arnoldi", "lanczos"])
@pytest.mark.parametrize("t", [0.5, -0.7j, 0.3 - 0.4j])
def test_expv_against_oracle_and_truth(eu, natural, t, sym):
    n, m = 300, 30
    A, b = (kc.scattered_sym(n) if sym else kc.sell5(n)), kc.cvector(n)
    op = eu.MIOperator(A, natural)
    w = eu.expv(t, op, b, m=m, keep_real=True)
    st = eu.expv.last_stats
    assert st["real_operator"] and st["path"] == ["two_kernel"] and st["m"] == m, st
    assert w.dtype == np.complex128
    close(w, ko.expv(t, A, b, m=m), TOL, "realop expv t=%s sym=%s vs oracle" % (t, sym))
    close(w, sl.expm(t * kc.as_dense(A).astype(np.complex128)) @ b, TOL_TRUTH, "realop expv t=%s sym=%s vs expm(tA) b" % (t, sym))


@pytest.mark.parametrize("t", [0.5, -0.7j, 0.3 - 0.4j])
def test_expv_float32_operator(eu, t):
    n, m = 300, 30
    A, b = kc.sell5(n, np.float32), kc.cvector(n, np.float32)
    w = eu.expv(t, eu.MIOperator(A), b, m=m, keep_real=True)
    assert eu.expv.last_stats["real_operator"] and w.dtype == np.complex64
    close(w, ko.expv(t, A.astype(np.float64), b.astype(np.complex128), m=m), TOL32, "realop expv f32 t=%s vs oracle" % (t,))


def test_expv_out_may_alias_b(eu, torch):
    n, m, t = 300, 30, -0.7j
    A, b = kc.sell5(n), kc.cvector(n)
    op = eu.MIOperator(A)
    want = eu.expv(t, op, b, m=m, keep_real=True)
    h = b.copy()
    assert eu.expv(t, op, h, m=m, out=h, keep_real=True) is h and np.array_equal(h, want)
    d = torch.from_numpy(b).cuda()
    assert eu.expv(t, op, d, m=m, out=d, keep_real=True) is d and np.array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize("born", ["lincomb", "adjoint"])
def test_expv_on_operators_that_cannot_be_promoted(eu, born):
    n, m, t = 300, 30, -0.7j
    A0, A1, b = kc.sell5(n), kc.gdia(n), kc.cvector(n)
    if born == "lincomb":
        op = eu.MIOperator(A0) + 0.3 * eu.MIOperator(A1)
        A = (A0 + 0.3 * A1).tocsr()
    else:
        op = eu.MIOperator(A0).adjoint()
        A = A0.T.tocsr()
    assert op.dtype == np.float64
    with pytest.raises(TypeError, match="keeps no source to convert"):
        eu.expv(t, op, b, m=m)                      # the default promotes through astype, as before
    w = eu.expv(t, op, b, m=m, keep_real=True)
    assert eu.expv.last_stats["real_operator"]
    close(w, ko.expv(t, A, b, m=m), TOL, "realop expv on a %s-born operator" % born)


# ---- expv_timestep / phiv_timestep ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("p", [0, 2])
def test_timestep_against_oracle(eu, p, adaptive):
    n = 300
    A = kc.sell5(n)
    B = np.asfortranarray(np.stack([kc.cvector(n, seed=40 + k) for k in range(p + 1)], axis=1))
    ts = np.linspace(0.5, 3.5, 7)
    op = eu.MIOperator(A)
    arg = B[:, 0].copy() if p == 0 else B
    st, so = {}, {}
    if p == 0:
        U = eu.expv_timestep(ts.copy(), op, arg, adaptive=adaptive, tol=1e-9, stats=st, keep_real=True)
        Uo = ko.expv_timestep(ts.copy(), A, arg, adaptive=adaptive, tol=1e-9, stats=so)
    else:
        U = eu.phiv_timestep(ts.copy(), op, arg, adaptive=adaptive, tol=1e-9, stats=st, keep_real=True)
        Uo = ko.phiv_timestep(ts.copy(), A, arg, adaptive=adaptive, tol=1e-9, stats=so)
    assert np.asarray(U).dtype == np.complex128 and np.asarray(U).shape == (n, 7)
    assert st["num_timesteps"] == so["num_timesteps"] and st["m"] == so["m"], (st, so)
    close(U, Uo, TOL, "realop timestep p=%d adaptive=%s vs oracle" % (p, adaptive))


def test_timestep_keep_real_is_needed_for_combined_operators(eu):
    n = 300
    op = eu.MIOperator(kc.sell5(n)) + 0.3 * eu.MIOperator(kc.gdia(n))
    b = kc.cvector(n)
    with pytest.raises(TypeError, match="keeps no source to convert"):
        eu.expv_timestep(np.array([0.2, 0.4]), op, b)
    U = eu.expv_timestep(np.array([0.2, 0.4]), op, b, tol=1e-9, keep_real=True)
    close(U, ko.expv_timestep(np.array([0.2, 0.4]), (kc.sell5(n) + 0.3 * kc.gdia(n)).tocsr(), b, tol=1e-9), TOL, "realop expv_timestep on a lincomb-born operator")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _raw_arnoldi(eu, Ks, op, b):
    from exponentialutilities_jl_amd import _lib as L
    o = L.ArnoldiOpts()
    L.load().expv_mi_arnoldi_opts_default(C.byref(o))
    o.m = 5
    code = L.load().expv_mi_arnoldi(Ks._h, op._h, b.ctypes.data, L.HOST, C.byref(o))
    msg = L.load().expv_mi_last_error(Ks.ctx._h)
    return code, (msg or b"").decode()


@pytest.mark.parametrize("opdt,T", [(np.float64, np.complex64), (np.float32, np.complex128), (np.complex128, np.float64),
                                    (np.complex128, np.complex64)], ids=["f64-c32", "f32-c64", "c64-f64", "c64-c32"])
def test_mismatched_pairs_keep_their_status_and_message(eu, opdt, T):
    n = 129
    op = eu.MIOperator(kc.sell5(n).astype(opdt))
    Ks = eu.KrylovSubspace(T, T, n, 5)
    code, msg = _raw_arnoldi(eu, Ks, op, np.ones(n, dtype=T))
    assert code == 2 and "operator dtype must equal the subspace dtype T" in msg, (code, msg)


def test_refused_entries_say_so(eu):
    from exponentialutilities_jl_amd import _lib as L
    n, p = 129, 1
    lib = L.load()
    op = eu.MIOperator(kc.sym_sell(n))
    o = L.ArnoldiOpts()
    lib.expv_mi_arnoldi_opts_default(C.byref(o))
    o.m = 5
    Ka = eu.KrylovSubspace(np.complex128, np.complex128, n, 5, augmented=p)
    B = np.zeros((n, p), dtype=np.complex128, order="F")
    w = kc.cvector(n)
    waug = (C.c_double * p)()
    code = lib.expv_mi_arnoldi_aug(Ka._h, op._h, B.ctypes.data, n, p, L.HOST, w.ctypes.data, L.HOST, waug, 0.1, 1.0, C.byref(o))
    msg = lib.expv_mi_last_error(Ka.ctx._h).decode()
    assert code == 2 and msg.endswith("arnoldi_aug: real operator with complex vectors is not supported here"), (code, msg)
    Ke = eu.KrylovSubspace(np.complex128, np.float64, n, 5)
    out = np.empty(n, dtype=np.complex128)
    code = lib.expv_mi_expv_error_estimate(Ke._h, op._h, 0.0, -0.5, w.ctypes.data, L.HOST, out.ctypes.data, L.HOST, 1e-8, 1e-4, 5, 1)
    msg = lib.expv_mi_last_error(Ke.ctx._h).decode()
    assert code == 2 and msg.endswith("expv_error_estimate: real operator with complex vectors is not supported here"), (code, msg)
    # the new entries refuse what is not theirs
    opc = eu.MIOperator(kc.sell5(n).astype(np.complex128))
    st = L.ExpvStats()
    code = lib.expv_mi_expv_realop(opc.ctx._h, opc._h, 0.0, -0.5, w.ctypes.data, L.HOST, out.ctypes.data, L.HOST, C.byref(o), C.byref(st))
    assert code == 2 and "expv_realop" in lib.expv_mi_last_error(opc.ctx._h).decode()


# ---- unchanged behaviour --------------------------------------------------------------------------------------------------------------
def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def default_keyword_results(eu):
    """expv(t, A_real, b_complex) with the default keyword on fixed inputs: name -> (digest of the result, real_operator)"""
    out = {}
    for name, A in (("sell5_2001", kc.sell5(2001)), ("gdia_1000", kc.gdia())):      # (two-kernel step: sums in a fixed order)
        b = kc.cvector(A.shape[0])
        for t in (0.5, -0.7j):
            w = eu.expv(t, A, b, m=30)
            out["%s t=%s" % (name, t)] = (_digest(w), bool(eu.expv.last_stats["real_operator"]))
    return out


def test_default_keyword_promotes_as_before_bit_for_bit(eu):
    """the record in tests/golden/krylov_realop_default_digests.json was taken with the library of the parent commit
    (profiles/krylov_realop_digests.txt)"""
    got = default_keyword_results(eu)
    assert not any(real_op for _, real_op in got.values())
    with open(os.path.join(ROOT, "tests", "golden", "krylov_realop_default_digests.json")) as f:
        want = json.load(f)
    assert {k: v[0] for k, v in got.items()} == want
