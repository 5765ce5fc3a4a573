"""exp(tA)B for a block of columns by the truncated Taylor series on the device (expv_mi_expv_taylor_block, eu.expv_taylor_block).

The contract is equality with the single call: column k of the block's result is BYTE FOR BYTE eu.expv_taylor(t, A, B[:, k]), and its
(applications, early_stages, nonfinite_stage) and |F|_inf are that call's.  Values are checked where the single call's are: column 0 of
the n = 1000 cases against scipy.linalg.expm(tA) b with the bar of tests/test_gpu_expv_taylor.py (its truths are shared)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import expv_taylor_cases as tc
from tests import test_gpu_expv_taylor as single
from tests._util import C2_OFFSETS, C2_VALS, banded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_N = single.SMALL_N
NCOLS = (1, 2, 3, 4, 5, 8, 9, 17)
PANEL = 8


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


def std_block(n, p, T):
    """columns chosen to stop at different terms: random, constant, e_1, zero, 0.001 x random, the rest random (column-major)"""
    T = np.dtype(T)
    B = np.empty((n, p), dtype=T, order="F")
    for k in range(p):
        B[:, k] = tc.vector(n, T, seed=k)
    if p > 1:
        B[:, 1] = 1.0
    if p > 2:
        B[:, 2] = 0.0
        B[0, 2] = 1.0
    if p > 3:
        B[:, 3] = 0.0
    if p > 4:
        B[:, 4] = T.type(0.001) * tc.vector(n, T, seed=4)
    return B


def bits(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint8)


def single_ref(eu, t, op, b, **kw):
    w, i = eu.expv_taylor(t, op, np.ascontiguousarray(b), return_info=True, **kw)
    return np.asarray(w), (i["applications"], i["early_stages"], i["nonfinite_stage"]), i


def assert_equals_singles(eu, t, op, B, W, info, refs=None, **kw):
    """every column of W and of the per-column info against the single call on that column"""
    n, p = B.shape
    W = np.asarray(W)
    assert W.shape == (n, p) and W.dtype == B.dtype
    for k in range(p):
        wk, ck, ik = refs[k] if refs is not None else single_ref(eu, t, op, B[:, k], **kw)
        assert np.array_equal(bits(W[:, k]), bits(wk)), "column %d of %d: other bits than the single call" % (k, p)
        assert (info["applications"][k], info["early_stages"][k], info["nonfinite_stage"][k]) == ck, (k, info, ck)
        assert np.array_equal(np.float64(info["normF"][k]).view(np.uint64), np.float64(ik["normF"]).view(np.uint64)) or (
            np.isnan(info["normF"][k]) and np.isnan(ik["normF"])), (k, info["normF"][k], ik["normF"])
        assert (info["m"], info["s"], info["alpha"], info["mu"]) == (ik["m"], ik["s"], ik["alpha"], ik["mu"])
    assert info["applications_total"] == sum(info["applications"])
    assert info["host_reads"] <= 2, info


def assert_block_path(info, p):
    panels = (p + PANEL - 1) // PANEL
    assert info["path"] == 1, info
    assert info["launches"] == panels * info["m"] * info["s"], info
    assert info["worked_launches"] <= info["launches"]


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.random8], ids=["tridiagonal", "random8"])
def test_every_column_equals_its_single_call(eu, mk, T, n):
    A = mk(n, T)
    op = eu.MIOperator(A)
    B = std_block(n, max(NCOLS), T)
    for ct in single.t_variants(T):
        t = tc.t_for(A, single.alpha_for(mk, T), ct)
        refs = [single_ref(eu, t, op, B[:, k]) for k in range(B.shape[1])]
        for p in NCOLS:
            Bp = np.asfortranarray(B[:, :p])
            W, info = eu.expv_taylor_block(t, op, Bp, return_info=True)
            assert_equals_singles(eu, t, op, Bp, W, info, refs=refs)
            assert_block_path(info, p)


def test_masking_is_exercised(eu):
    """columns of one panel that stop at different terms: the later launches of a stage run with some of them masked"""
    n, T = 257, np.float64
    A = tc.laplacian(n, T)
    op = eu.MIOperator(A)
    B = std_block(n, 8, T)
    t = tc.t_for(A, 40.0)
    W, info = eu.expv_taylor_block(t, op, B, return_info=True)
    assert_equals_singles(eu, t, op, B, W, info)
    apps = info["applications"]
    print("[taylor block] applications per column:", apps, "worked launches", info["worked_launches"], "of", info["launches"])
    assert apps[3] == 0 and len(set(apps)) >= 2, apps
    live = [a for k, a in enumerate(apps) if k != 3]
    assert len(set(live)) >= 2, "no two non-zero columns stopped at different terms: %r" % (apps,)
    # a launch does work as long as one column of its panel is live
    assert max(apps) <= info["worked_launches"] <= min(info["launches"], sum(apps)), info


def callback_operator(eu, n):
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
    return A, op, float(abs(A).sum(axis=1).max()), (sop, cbl)


def value_check_of_column_0(eu, tables, name, A, b, t, w, opnorm=None):
    """the bar of tests/test_gpu_expv_taylor.py: device error <= 8 x max(restatement error, eps) against scipy.linalg.expm(tA) b"""
    T = np.dtype(A.dtype)
    tab = tc.table_of(T, 0)
    mu, alpha, _ = tc.shift_norm(A, t)
    if opnorm is not None:
        mu, alpha = 0.0, abs(t) * opnorm
    Fr, _ = tc.restated(t, A, b, T, alpha, tables[tab], tc.TOL[tab], mu)
    truth = single.truth_of((name, T.name, A.shape[0], complex(t)), A, b, t)
    e_rest, e_dev = tc.relmax(Fr, truth), tc.relmax(w, truth)
    print("[taylor block] %s %s: restated %.2e device %.2e" % (name, T.name, e_rest, e_dev))
    assert e_dev <= single.BAR * max(e_rest, tc.eps_of(T)), "%s: device %.3e > %g x max(restatement %.3e, eps)" % (name, e_dev, single.BAR, e_rest)


@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.penta, tc.random8, tc.powerlaw, tc.dense], ids=["tridiagonal", "pentadiagonal", "random8", "powerlaw", "dense"])
def test_n1000_every_operator_form(eu, tables, mk, T):
    n, p = 1000, 5
    A = mk(n, T)
    op = eu.MIOperator(A)
    B = std_block(n, p, T)
    t = tc.t_for(A, single.alpha_for(mk, T))
    W, info = eu.expv_taylor_block(t, op, B, return_info=True)
    assert_equals_singles(eu, t, op, B, W, info)
    want = {tc.laplacian: 1, tc.penta: 1, tc.random8: 1, tc.powerlaw: 2, tc.dense: 2}[mk]
    assert info["path"] == want, info
    if want == 1:
        assert_block_path(info, p)
    else:
        assert info["launches"] == p * info["m"] * info["s"], info
    value_check_of_column_0(eu, tables, mk.__name__, A, B[:, 0].copy(), t, np.asarray(W)[:, 0])


def test_n1000_compiled_callback_with_opnorm(eu, tables):
    n, p = 1000, 5
    A, op, opnorm, keep = callback_operator(eu, n)
    B = std_block(n, p, np.float64)
    t = 20.0 / opnorm
    W, info = eu.expv_taylor_block(t, op, B, opnorm=opnorm, return_info=True)
    assert_equals_singles(eu, t, op, B, W, info, opnorm=opnorm)
    assert info["path"] == 2 and info["launches"] == p * info["m"] * info["s"], info
    value_check_of_column_0(eu, tables, "callback", A, B[:, 0].copy(), t, np.asarray(W)[:, 0], opnorm=opnorm)
    with pytest.raises(eu.ExpvMIError) as ei:      # a callback without its bound
        eu.expv_taylor_block(t, op, B)
    assert ei.value.kind == "ArgumentError" and "opnorm" in str(ei.value)
    del keep


@pytest.mark.parametrize("mk", [tc.random8, tc.powerlaw], ids=["block", "columns"])
def test_layouts_padding_and_aliasing_give_the_same_bytes(eu, torch, mk):
    n, p, T = 129, 5, np.float64
    A = mk(n, T)
    op = eu.MIOperator(A)
    B = std_block(n, p, T)
    t = tc.t_for(A, 30.0)
    want = np.asarray(eu.expv_taylor_block(t, op, B))
    assert want.flags.f_contiguous
    for k in range(p):
        assert np.array_equal(bits(want[:, k]), bits(single_ref(eu, t, op, B[:, k])[0]))

    def same(W):
        return np.array_equal(bits(np.asarray(W)), bits(want))

    # numpy, row-major: the result comes back in B's order
    Wc = eu.expv_taylor_block(t, op, np.ascontiguousarray(B))
    assert Wc.flags.c_contiguous and same(Wc)
    # padded leading dimensions on the host, NaN in the padding of B and W, mixed layouts of B and W
    for xp in ("numpy", "torch-device"):
        colB, colW = np.full((n + 3, p), np.nan, order="F"), np.full((n + 5, p), np.nan, order="F")
        rowB, rowW = np.full((n, p + 2), np.nan, order="C"), np.full((n, p + 3), np.nan, order="C")
        colB[:n] = B
        rowB[:, :p] = B
        for Bbig, Wbig, cut in ((colB, colW, "rows"), (rowB, rowW, "cols"), (colB, rowW, "mixed")):
            if xp == "torch-device":
                Bbig = torch.as_tensor(Bbig.copy(order="C")).cuda() if Bbig.flags.c_contiguous else torch.as_tensor(np.ascontiguousarray(Bbig.T)).cuda().t()
                Wbig = torch.as_tensor(Wbig.copy(order="C")).cuda() if Wbig.flags.c_contiguous else torch.as_tensor(np.ascontiguousarray(Wbig.T)).cuda().t()
            Bv = Bbig[:n] if Bbig.shape[0] > n else Bbig[:, :p]
            Wv = Wbig[:n] if Wbig.shape[0] > n else Wbig[:, :p]
            before = np.array(Bbig.cpu().numpy() if xp == "torch-device" else Bbig, copy=True)
            out = eu.expv_taylor_block_(Wv, t, op, Bv)
            assert out is Wv
            Wh = Wbig.cpu().numpy() if xp == "torch-device" else Wbig
            got = Wh[:n] if Wh.shape[0] > n else Wh[:, :p]
            pad = Wh[n:] if Wh.shape[0] > n else Wh[:, p:]
            assert same(got), (xp, cut)
            assert pad.size > 0 and np.all(np.isnan(pad)), "the padding of W was written (%s, %s)" % (xp, cut)
            after = Bbig.cpu().numpy() if xp == "torch-device" else Bbig
            assert np.array_equal(before, after, equal_nan=True), "B was changed (%s, %s)" % (xp, cut)
    # a contiguous torch (n, p) device tensor, W is B
    X = torch.as_tensor(np.ascontiguousarray(B)).cuda()
    assert X.is_contiguous()
    out, info = eu.expv_taylor_block_(X, t, op, X, return_info=True)
    assert out is X and same(X.cpu().numpy())
    assert info["path"] == (1 if mk is tc.random8 else 2)
    # column-major device tensor, W is B
    Xf = torch.as_tensor(np.ascontiguousarray(B.T)).cuda().t()
    assert eu.expv_taylor_block_(Xf, t, op, Xf) is Xf and same(Xf.cpu().numpy())
    # device result of the allocating form lives where B does, in B's order
    Wd = eu.expv_taylor_block(t, op, torch.as_tensor(np.ascontiguousarray(B)).cuda())
    assert torch.is_tensor(Wd) and Wd.is_cuda and Wd.is_contiguous() and same(Wd.cpu().numpy())
    # torch in host memory, both orders; numpy W is B
    for Bt in (torch.as_tensor(np.array(B, order="C")), torch.as_tensor(np.array(B.T, order="C")).t()):      # (copies: W is B below)
        Wt = eu.expv_taylor_block(t, op, Bt)
        assert torch.is_tensor(Wt) and not Wt.is_cuda and same(Wt.numpy())
        assert eu.expv_taylor_block_(Bt, t, op, Bt) is Bt and same(Bt.numpy())
    for order in ("C", "F"):
        Bn = np.array(B, order=order)
        assert eu.expv_taylor_block_(Bn, t, op, Bn) is Bn and same(Bn)
    # a DeviceArray (column-major, owned by the library)
    Bd = eu.DeviceArray.from_host(B)
    Wd = eu.expv_taylor_block(t, op, Bd)
    assert isinstance(Wd, eu.DeviceArray) and same(Wd.to_host())


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_reordered_operator_answers_in_the_callers_ordering(eu, T):
    n, p = 1000, 3
    ctx = eu.Context()
    ctx.set_option("reorder", 2)
    A, _ = tc.shuffled_band(n, T)
    A.sort_indices()
    op = eu.MIOperator(A, ctx)
    assert op.reorder_info["reordered"], op.reorder_info
    B = std_block(n, p, T)
    t = tc.t_for(A, 40.0)
    W, info = eu.expv_taylor_block(t, op, B, return_info=True)
    assert_equals_singles(eu, t, op, B, W, info)
    assert_block_path(info, p)
    # the rows are the caller's: the same operator in its natural ordering agrees to rounding
    Wn = np.asarray(eu.expv_taylor_block(t, eu.MIOperator(A), B))
    assert tc.relmax(np.asarray(W), Wn) <= 1e3 * tc.eps_of(T)


@pytest.mark.parametrize("mk,path", [(tc.random8, 1), (tc.powerlaw, 2)], ids=["block", "columns"])
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_one_column_with_an_infinite_entry(eu, mk, path, T):
    n, p = 257, 5
    A = mk(n, T)
    op = eu.MIOperator(A)
    t = tc.t_for(A, 40.0)
    good = std_block(n, p, T)
    B = good.copy(order="F")
    B[n // 3, 0] = np.inf
    W, info = eu.expv_taylor_block(t, op, B, return_info=True)
    assert info["path"] == path
    assert info["nonfinite_stage"][0] >= 1 and info["nonfinite_columns"] == 1, info
    assert all(s == 0 for s in info["nonfinite_stage"][1:]), info
    assert not np.all(np.isfinite(np.asarray(W)[:, 0])) and np.all(np.isfinite(np.asarray(W)[:, 1:]))
    assert not np.isfinite(info["normF_max"])
    assert_equals_singles(eu, t, op, B, W, info)
    W2, info2 = eu.expv_taylor_block(t, op, good, return_info=True)      # the context and the operator are as good as before
    assert info2["nonfinite_columns"] == 0
    assert_equals_singles(eu, t, op, good, W2, info2)


@pytest.mark.parametrize("T", tc.DTYPES)
def test_all_zero_block_applies_nothing(eu, T):
    n, p = 257, 5
    A = tc.random8(n, T)
    W, info = eu.expv_taylor_block(tc.t_for(A, 40.0), A, np.zeros((n, p), dtype=T), return_info=True)
    assert not np.any(np.asarray(W)) and info["applications"] == [0] * p and info["applications_total"] == 0
    assert info["launches"] == info["m"] * info["s"] > 0 and info["worked_launches"] == 0, info
    assert info["normF"] == [0.0] * p and info["nonfinite_columns"] == 0


def test_more_workgroups_than_compute_units(eu):
    """n = 70 001: the ticket's last arrival is not the last workgroup launched"""
    n, p, T = 70001, 8, np.float64
    A = tc.laplacian(n, T)
    op = eu.MIOperator(A)
    B = std_block(n, p, T)
    t = tc.t_for(A, 10.0)
    W, info = eu.expv_taylor_block(t, op, B, return_info=True)
    assert_equals_singles(eu, t, op, B, W, info)
    assert_block_path(info, p)


@pytest.mark.parametrize("mk,path", [(tc.random8, 1), (tc.laplacian, 1), (tc.powerlaw, 2)], ids=["sell", "dia", "overflow"])
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_two_calls_give_the_same_bits(eu, mk, path, T):
    n, p = 1000, 9
    A = mk(n, T)
    op = eu.MIOperator(A)
    B = std_block(n, p, T)
    t = tc.t_for(A, 30.0)
    W1, i1 = eu.expv_taylor_block(t, op, B, return_info=True)
    W2, i2 = eu.expv_taylor_block(t, op, B, return_info=True)
    assert i1["path"] == path
    assert repr(i1) == repr(i2)      # (repr: a NaN would compare unequal to itself)
    assert np.array_equal(bits(W1), bits(W2))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_max_matvecs_at_and_below_the_need(eu):
    n, p = 257, 3
    A = tc.penta(n, np.float64)
    op = eu.MIOperator(A)
    B = std_block(n, p, np.float64)
    t = tc.t_for(A, 40.0)
    want, info = eu.expv_taylor_block(t, op, B, return_info=True)
    need = info["m"] * info["s"]
    W = np.full((n, p), 7.0, order="F")
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_block_(W, t, op, B, max_matvecs=need - 1)
    msg = str(ei.value)
    assert ei.value.kind == "ArgumentError" and "alpha" in msg and "m* = %d" % info["m"] in msg and "s = %d" % info["s"] in msg, msg
    assert np.all(W == 7.0), "a refused call must leave W alone"
    Wd = eu.DeviceArray.from_host(W)
    with pytest.raises(eu.ExpvMIError):
        eu.expv_taylor_block_(Wd, t, op, eu.DeviceArray.from_host(B), max_matvecs=need - 1)
    assert np.all(Wd.to_host() == 7.0), "a refused call must leave a device W alone"
    assert np.array_equal(bits(eu.expv_taylor_block(t, op, B, max_matvecs=need)), bits(want))


def test_real_operator_refuses_a_complex_t(eu):
    A, B = tc.penta(65, np.float64), std_block(65, 3, np.float64)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_block(0.5 + 0.25j, A, B)
    assert ei.value.kind == "ArgumentError"
    for bad in (2, -1):
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.expv_taylor_block(0.5, A, B, precision=bad)
        assert ei.value.kind == "ArgumentError"


def test_bad_arguments_are_refused_before_any_device_work(eu):
    n, p = 65, 3
    A = tc.penta(n, np.float64)
    op = eu.MIOperator(A)
    B = std_block(n, p, np.float64)
    big = np.full((n + 4) * p, 7.0)
    lib, L = eu.api.L.load(), eu.api.L
    info, dinfo = (C.c_int64 * 8)(), (C.c_double * 4)()

    def call(Bp, ldb, ncols, bl, Wp, ldw, wl, b_loc=L.HOST, w_loc=L.HOST):
        return lib.expv_mi_expv_taylor_block(op.ctx._h, op._h, 0.1, 0.0, Bp, ldb, ncols, bl, b_loc, Wp, ldw, wl, w_loc, 0, 0, 0.0, info, dinfo, None, None)

    Bp, Wp = B.ctypes.data, big.ctypes.data
    COL, ROW = L.BLOCK_COL_MAJOR, L.BLOCK_ROW_MAJOR
    cases = {"ncols < 0": (Bp, n, -1, COL, Wp, n, COL), "layout of B": (Bp, n, p, 2, Wp, n, COL), "layout of W": (Bp, n, p, COL, Wp, n, -1),
             "ldb, column-major": (Bp, n - 1, p, COL, Wp, n, COL), "ldw, column-major": (Bp, n, p, COL, Wp, n - 1, COL),
             "ldb, row-major": (Bp, p - 1, p, ROW, Wp, n, COL), "ldw, row-major": (Bp, n, p, COL, Wp, p - 1, ROW),
             "W inside B": (Bp, n, p, COL, Bp + 8, n, COL), "W is B in another layout": (Bp, n, p, COL, Bp, p, ROW),
             "W is B with another ld": (Wp, n, p, COL, Wp, n + 1, COL)}
    for name, args in cases.items():
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.api._check(call(*args), op.ctx._h)
        assert ei.value.kind == "ArgumentError" and "expv_taylor_block:" in str(ei.value), (name, str(ei.value))
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.api._check(call(Bp, n, p, COL, Wp, n, COL, b_loc=5), op.ctx._h)
    assert ei.value.kind == "ArgumentError"
    assert np.all(big == 7.0) and np.array_equal(B, std_block(n, p, np.float64))
    # overlapping views through the front end
    both = np.zeros((n + 1, p), order="F")
    both[:n] = B
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_block_(both[1:], 0.1, op, both[:n])
    assert ei.value.kind == "ArgumentError" and "overlaps" in str(ei.value)
    # nothing to do: no columns
    eu.api._check(call(Bp, n, 0, COL, Wp, n, COL), op.ctx._h)
    assert list(info) == [0] * 8 and np.all(big == 7.0)
    W0 = eu.expv_taylor_block(0.1, op, np.zeros((n, 0)))
    assert np.asarray(W0).shape == (n, 0)


def test_the_single_call_still_refuses_a_block(eu):
    A = tc.penta(65, np.float64)
    with pytest.raises(eu.api.DimensionMismatch):
        eu.expv_taylor(0.1, A, std_block(65, 3, np.float64))
