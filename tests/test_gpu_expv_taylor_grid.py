"""exp(ts[k] t A) b on a time grid in one sweep of the truncated Taylor series (expv_mi_expv_taylor_grid, eu.expv_taylor_grid).

Truth per output: scipy.linalg.expm(r_k t A) b in fp64 / complex128 (tests/expv_taylor_grid_cases.py: one expm per output for
n <= 257, the product form on the grid's lattice at n = 1000 (one expm per output where that form is beyond its gap limit), scipy's expm_multiply at n = 70001).  Bar, per output: the device's
error <= 8 x max(error of the numpy restatement run in the operator's element type on the same input, eps_T), both relative in the
max norm -- as the single call's tests have it.  Every case's figures go to profiles/expv_taylor_grid_parity.txt."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests import expv_taylor_cases as tc
from tests import expv_taylor_grid_cases as gc
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
        with open(os.path.join(ROOT, "profiles", "expv_taylor_grid_parity.txt"), "w") as f:
            f.write("# expv_taylor_grid against scipy.linalg.expm(r_k t A) b per output (n = 1000: its product form on the grid's lattice, `gap` = that\n"
                    "# form against the direct expm at r = 1/4, 1/2 and 1, the largest, in eps; n = 70001: scipy's expm_multiply): worst relative max-norm error over the outputs;\n"
                    "# bar per output = 8 x max(restatement, eps)\n")
            f.write("%-40s %-10s %4s %7s %3s %3s %4s %4s %5s %5s %5s %4s %10s %10s %6s\n" % ("case", "dtype", "prec", "alpha", "m*", "s", "q", "qmax", "apps", "terms", "accum",
                                                                                       "path", "restated", "device", "gap"))
            f.write("\n".join(_lines) + "\n")
    except OSError:
        pass


def alpha_for(mk, T):
    return 10.0 if (mk is tc.laplacian and np.dtype(T).kind == "c") else 40.0


def t_variants(T):
    return (False, True) if np.dtype(T).kind == "c" else (False,)


def bits(x):
    return np.ascontiguousarray(np.asarray(x)).view(np.uint8)


def expected_accum(info):
    per_stage = {}
    for st, kd in zip(info["stage"], info["kind"]):
        if kd == 1:
            per_stage[st] = per_stage.get(st, 0) + 1
    return info["m"] * sum(max(0, -(-c // 8) - 1) for c in per_stage.values()), max(per_stage.values(), default=0)


def check(eu, tables, name, A, b, t, r, truth, precision=0, op=None, path=None, opnorm=None, gap=float("nan"), truth_bar=None):
    """one grid call against the restatement and the truth, with every assertion of the issue; returns (W, info)"""
    T = np.dtype(A.dtype)
    tab = tc.table_of(T, precision)
    r = np.asarray(r, dtype=np.float64)
    mu, alpha, _ = tc.shift_norm(A, r.max() * t)
    if opnorm is not None:
        mu, alpha = 0.0, abs(r.max() * t) * opnorm
    Wr, ir = gc.restated_grid(t, r, A, b, T, alpha, tables[tab], tc.TOL[tab], mu)
    W, info = eu.expv_taylor_grid(r, A if op is None else op, b, t=t, precision=precision, opnorm=opnorm, return_info=True)
    W = np.asarray(W)
    assert W.dtype == T and W.shape == (A.shape[0], r.size)
    e_rest, e_dev = gc.relmax_columns(Wr, truth), gc.relmax_columns(W, truth)
    accum, qmax = expected_accum(info)
    _lines.append("%-40s %-10s %4d %7.3f %3d %3d %4d %4d %5d %5d %5d %4d %10.2e %10.2e %6.1f" % (
        name + " n=%d" % A.shape[0] + (" ct" if isinstance(t, complex) else ""), T.name, precision, info["alpha"], info["m"], info["s"], r.size, info["qmax"],
        info["applications"], info["launches"], info["accumulate_launches"], info["path"], max(e_rest, default=0.0), max(e_dev, default=0.0),
        gap / tc.eps_of(tc.wide(T))))
    print("[taylor grid]", _lines[-1])
    # plan and counters
    assert (info["m"], info["s"]) == (ir["m"], ir["s"]) == eu.host_taylor_params(info["alpha"], tab)
    assert info["stage"] == ir["stage"] and info["kind"] == ir["kind"]
    assert all(abs(a - c) <= 1 for a, c in zip(info["terms"], ir["terms"])), (info["terms"], ir["terms"])
    assert info["host_reads"] <= 2 and info["launches"] == info["m"] * info["s"], info
    assert info["accumulate_launches"] == accum and info["qmax"] == qmax, (info, accum, qmax)
    assert info["applications"] <= info["launches"] and info["nonfinite_stage"] == 0
    if path is not None:
        assert info["path"] == path, info
    # values, output by output
    for k in range(r.size):
        ref = e_rest[k] if truth_bar is None else truth_bar[k]
        assert e_dev[k] <= BAR * max(ref, tc.eps_of(T)), "%s output %d (r = %g, kind %d): device %.3e > %g x max(restatement %.3e, eps)" % (
            name, k, r[k], info["kind"][k], e_dev[k], BAR, ref)
    return W, info


def small_truth(mk, T, n, t, A, b, r):
    key = (mk.__name__, np.dtype(T).name, n, complex(t), r.tobytes())
    if key not in _truths:
        _truths[key] = gc.truth_columns(A, b, t, r)
    return _truths[key]


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.random8], ids=["tridiagonal", "random8"])
def test_slice_boundaries(eu, tables, mk, T, n):
    A, b = mk(n, T), tc.vector(n, T)
    r = gc.rand13()
    for ct in t_variants(T):
        t = tc.t_for(A, alpha_for(mk, T), ct)
        check(eu, tables, mk.__name__ + " rand13", A, b, t, r, small_truth(mk, T, n, t, A, b, r))


@pytest.mark.parametrize("T", tc.DTYPES)
@pytest.mark.parametrize("mk", [tc.laplacian, tc.penta, tc.random8, tc.powerlaw, tc.dense], ids=["tridiagonal", "pentadiagonal", "random8", "powerlaw", "dense"])
def test_n1000_every_operator_form_and_panel_count(eu, tables, mk, T):
    n = 1000
    A, b = mk(n, T), tc.vector(n, T)
    want = {tc.laplacian: 1, tc.penta: 1, tc.random8: 1, tc.powerlaw: 2, tc.dense: 2}[mk]
    t = tc.t_for(A, alpha_for(mk, T))
    op = eu.MIOperator(A)
    wide64 = np.dtype(T).itemsize >= (16 if np.dtype(T).kind == "c" else 8)
    seen = set()
    for precision in (0, 1) if wide64 else (0,):
        tab = tc.table_of(T, precision)
        s = tc.params(tc.shift_norm(A, t)[1], tables[tab])[1]
        grids = [("lin40", gc.lin40(), None, 40)] + [("panels%d" % i, r, c, s * gc.PANEL_SLOTS) for i, (r, c) in enumerate(gc.panel_grids(s))]
        for gname, r, counts, L in grids:
            if (L,) not in _truths.setdefault((mk.__name__, np.dtype(T).name), {}):
                _truths[(mk.__name__, np.dtype(T).name)][(L,)] = gc.lattice_truth(A, b, t, L)
            X, gap = _truths[(mk.__name__, np.dtype(T).name)][(L,)]
            if counts is not None:
                stage, _, kind = eu.host_taylor_grid_plan(s, r)
                assert [int(np.sum((stage == i) & (kind == 1))) for i in range(s)] == counts
                seen.update(counts)
            check(eu, tables, "%s %s" % (mk.__name__, gname), A, b, t, r, gc.grid_truth(A, b, t, r, L, (X, gap)), precision=precision, op=op, path=want, gap=gap)
    assert seen >= set(gc.PANEL_COUNTS), seen      # remainder panels of 2, 4 and 8 columns, one and two extra panels


@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_more_workgroups_than_compute_units(eu, tables, T):
    """n = 70 001 (the single call's size for this): values against scipy's expm_multiply on the CPU, output by output; bar from its own
    agreement with the restatement."""
    n = 70001
    A, b = tc.laplacian(n, T), tc.vector(n, T)
    t = tc.t_for(A, 10.0)
    r = np.array([0.37, 1.0, 0.0, 0.5, 0.81, 0.12, 0.93, 0.5, 0.66, 0.25, 0.07])      # 9 interior outputs in one stage when s = 1 .. 2
    ref = np.stack([spl.expm_multiply((x * t) * A, b) if x > 0 else b for x in r], axis=1)
    mu, alpha, _ = tc.shift_norm(A, t)
    Wr = gc.restated_grid(t, r, A, b, T, alpha, tables[0], tc.TOL[0], mu)[0]
    check(eu, tables, "laplacian", A, b, t, r, ref, path=1, truth_bar=gc.relmax_columns(Wr, ref))


# ---- bit for bit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("mk,path", [(tc.random8, 1), (tc.laplacian, 1), (tc.powerlaw, 2), (tc.dense, 2)], ids=["sell", "dia", "overflow", "dense"])
@pytest.mark.parametrize("T", tc.DTYPES)
def test_bits_of_the_single_call_of_b_of_duplicates_and_of_permutations(eu, mk, path, T, precision):
    n = 257
    A, b = mk(n, T), tc.vector(n, T)
    op = eu.MIOperator(A)
    t = tc.t_for(A, alpha_for(mk, T), np.dtype(T).kind == "c")
    ts = gc.rand13() * 1.75
    ts[3] = ts.max()      # a second output at R
    R = float(ts.max())
    single = np.asarray(eu.expv_taylor(R * t, op, b, precision=precision))
    W, info = eu.expv_taylor_grid(ts, op, b, t=t, precision=precision, return_info=True)
    assert info["path"] == path and W.flags.f_contiguous
    for k in np.flatnonzero(ts == R):
        assert info["kind"][k] == 2 and np.array_equal(bits(W[:, k]), bits(single)), "an output at R is not the single call's result"
    assert np.array_equal(bits(eu.expv_taylor_grid(R, op, b, t=t, precision=precision)), bits(single)), "a scalar ts is the single call"
    k0 = int(np.flatnonzero(ts == 0.0)[0])
    assert info["kind"][k0] == 0 and info["stage"][k0] == -1 and np.array_equal(bits(W[:, k0]), bits(b))
    dup = [k for k in range(ts.size) if np.sum(ts == ts[k]) > 1 and ts[k] != R]
    assert len(dup) == 2 and np.array_equal(bits(W[:, dup[0]]), bits(W[:, dup[1]]))
    W2, info2 = eu.expv_taylor_grid(ts, op, b, t=t, precision=precision, return_info=True)
    assert info2 == info and np.array_equal(bits(W2), bits(W)), "two identical calls"
    perm = tc.rng_of(n, 3).permutation(ts.size)
    keep = ts.copy()
    W3 = eu.expv_taylor_grid(ts[perm], op, b, t=t, precision=precision)
    assert np.array_equal(ts, keep)
    assert np.array_equal(bits(W3), bits(W[:, perm])), "permuting ts must permute the columns, bit for bit"
    if np.dtype(T).kind != "c":      # all <= 0: the sign goes into t
        assert np.array_equal(bits(eu.expv_taylor_grid(-ts, op, b, t=-t, precision=precision)), bits(W))
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.expv_taylor_grid(np.where(np.arange(ts.size) == 1, -ts, ts), op, b, t=t)
        assert ei.value.kind == "ArgumentError"


# ---- layouts and locations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_padded_layouts_keep_their_padding(eu, T):
    n = 129
    A, b = tc.penta(n, T), tc.vector(n, T)
    op = eu.MIOperator(A)
    t, ts = tc.t_for(A, 30.0), gc.rand13()
    q = ts.size
    want = eu.expv_taylor_grid(ts, op, b, t=t)
    big = np.full((n + 3, q), 7.0, dtype=T, order="F")      # column-major, ldw = n + 3
    assert eu.expv_taylor_grid_(big[:n], ts, op, b, t=t) is not None
    assert np.array_equal(bits(big[:n]), bits(want)) and np.all(big[n:] == 7.0)
    wide = np.full((n, q + 2), 7.0, dtype=T, order="C")      # row-major, ldw = q + 2
    eu.expv_taylor_grid_(wide[:, :q], ts, op, b, t=t)
    assert np.array_equal(bits(wide[:, :q]), bits(want)) and np.all(wide[:, q:] == 7.0)


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_torch_device_block_and_device_born_operator(eu, torch, tables, T):
    n = 257
    A, b = tc.random8(n, T), tc.vector(n, T)
    t, ts = tc.t_for(A, 40.0), gc.rand13()
    At = torch.sparse_csr_tensor(torch.as_tensor(A.indptr.astype(np.int64)).cuda(), torch.as_tensor(A.indices.astype(np.int64)).cuda(),
                                 torch.as_tensor(A.data).cuda(), size=(n, n))
    op = eu.MIOperator(At)
    want, _ = check(eu, tables, "device CSR rand13", A, b, t, ts, small_truth(tc.random8, T, n, t, A, b, ts), op=op, path=1)
    x = torch.as_tensor(b).cuda()
    Wt = eu.expv_taylor_grid(ts, op, x, t=t)
    assert torch.is_tensor(Wt) and Wt.is_cuda and Wt.shape == (n, ts.size) and Wt.is_contiguous()
    assert np.array_equal(bits(Wt.cpu().numpy()), bits(want))
    Wh = np.empty((n, ts.size), dtype=T)      # a host block for a device vector
    eu.expv_taylor_grid_(Wh, ts, op, x, t=t)
    assert np.array_equal(bits(Wh), bits(want))
    pad = torch.full((n, ts.size + 3), 7.0, dtype=Wt.dtype, device="cuda")
    eu.expv_taylor_grid_(pad[:, :ts.size], ts, op, x, t=t)
    assert np.array_equal(bits(pad[:, :ts.size].cpu().numpy()), bits(want)) and bool((pad[:, ts.size:] == 7.0).all())


@pytest.mark.parametrize("T", tc.DTYPES)
def test_reordered_operator_answers_in_the_callers_ordering(eu, tables, T):
    n = 257
    ctx = eu.Context()
    ctx.set_option("reorder", 2)
    A, _ = tc.shuffled_band(n, T)
    A.sort_indices()
    b = tc.vector(n, T)
    op = eu.MIOperator(A, ctx)
    assert op.reorder_info["reordered"], op.reorder_info
    t, ts = tc.t_for(A, 40.0), gc.rand13()
    check(eu, tables, "shuffled band rand13", A, b, t, ts, gc.truth_columns(A, b, t, ts), op=op, path=1)


def stencil(eu, n, vals):
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
    sop = StencilOp(n, len(C2_OFFSETS), (C.c_int * 8)(*C2_OFFSETS), (C.c_double * 8)(*vals))
    op = eu.MIOperator(None, eu.default_context(), matvec_c=(cbl.stencil_matvec, C.addressof(sop)), shape=(n, n), dtype=np.float64, ishermitian=False)
    return op, sop


def test_compiled_callback_with_opnorm(eu, tables):
    n = 257
    op, sop = stencil(eu, n, C2_VALS)
    A = banded(n, C2_OFFSETS, C2_VALS)
    b = tc.vector(n, np.float64)
    opnorm = float(abs(A).sum(axis=1).max())
    t, ts = 20.0 / opnorm, gc.rand13()
    check(eu, tables, "callback rand13", A, b, t, ts, gc.truth_columns(A, b, t, ts), op=op, path=2, opnorm=opnorm)
    W = np.full((n, ts.size), 7.0, order="F")
    with pytest.raises(eu.ExpvMIError) as ei:      # a callback without its bound
        eu.expv_taylor_grid_(W, ts, op, b, t=t)
    assert ei.value.kind == "ArgumentError" and "opnorm" in str(ei.value) and np.all(W == 7.0)
    del sop


# ---- edges -------------------------------------------------------------------------------------------------------------------
def raw(eu, op, r, nt, b, W, ldw, layout=0, b_loc=0, w_loc=0, t=(1.0, 0.0), precision=0, max_matvecs=0, opnorm=0.0):
    """the C entry point as it is; returns (status, message, info)"""
    lib = eu.api.L.load()
    info, dinfo = (C.c_int64 * 10)(*([7] * 10)), (C.c_double * 4)(*([7.0] * 4))
    rr = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    code = lib.expv_mi_expv_taylor_grid(op.ctx._h, op._h, t[0], t[1], None if rr is None else rr.ctypes.data_as(C.POINTER(C.c_double)), nt,
                                        None if b is None else b.ctypes.data, b_loc, None if W is None else W.ctypes.data, ldw, layout, w_loc, precision,
                                        max_matvecs, opnorm, info, dinfo, None)
    msg = lib.expv_mi_last_error(op.ctx._h)
    return code, (msg.decode() if isinstance(msg, bytes) else str(msg)), list(info)


def test_nothing_to_do(eu):
    n = 65
    A, b = tc.penta(n, np.float64), tc.vector(n, np.float64)
    op = eu.MIOperator(A)
    W = eu.expv_taylor_grid(np.zeros(0), op, b)
    assert W.shape == (n, 0)
    code, _, info = raw(eu, op, None, 0, b, None, 1)
    assert code == 0 and info == [0] * 10
    h = C.c_void_p()      # n = 0
    ctx, lib = eu.default_context(), eu.api.L.load()
    rp = np.zeros(1, dtype=np.int32)
    eu.api._check(lib.expv_mi_op_create_csr(ctx._h, eu.api.L.F64, 0, rp.ctypes.data, None, None, 4, 0, C.byref(h)), ctx._h)
    try:
        info = (C.c_int64 * 10)(*([7] * 10))
        r = np.ones(3)
        eu.api._check(lib.expv_mi_expv_taylor_grid(ctx._h, h, 1.0, 0.0, r.ctypes.data_as(C.POINTER(C.c_double)), 3, None, 0, None, 1, 0, 0, 0, 0, 0.0, info, None,
                                                   None), ctx._h)
        assert list(info) == [0] * 10
    finally:
        lib.expv_mi_op_destroy(h)


@pytest.mark.parametrize("T", tc.DTYPES)
def test_t_zero_and_R_zero_return_b(eu, T):
    n = 129
    A, b = tc.random8(n, T), tc.vector(n, T)
    for ts, t in ((gc.rand13(), 0.0), (np.zeros(5), 0.7)):
        W, info = eu.expv_taylor_grid(ts, A, b, t=t, return_info=True)
        assert all(np.array_equal(bits(W[:, k]), bits(b)) for k in range(ts.size))
        assert (info["m"], info["s"], info["applications"], info["launches"], info["alpha"]) == (0, 1, 0, 0, 0.0)


@pytest.mark.parametrize("T", tc.DTYPES)
def test_zero_vector_costs_no_application(eu, T):
    n = 257
    A = tc.random8(n, T)
    W, info = eu.expv_taylor_grid(gc.rand13(), A, np.zeros(n, dtype=T), t=tc.t_for(A, 40.0), return_info=True)
    assert not np.any(W) and info["applications"] == 0 and info["launches"] == info["m"] * info["s"] > 0
    assert info["terms"] == [0] * 13 and info["normF"] == 0.0 and info["nonfinite_stage"] == 0


@pytest.mark.parametrize("T", tc.DTYPES)
def test_shift_annihilates_a_multiple_of_the_identity(eu, T):
    n, t = 129, 0.75
    c = np.dtype(T).type(1.5 - 0.5j) if np.dtype(T).kind == "c" else np.dtype(T).type(1.5)
    A = (sp.identity(n, format="csr") * c).astype(T)
    b = tc.vector(n, T)
    ts = gc.rand13()
    W, info = eu.expv_taylor_grid(ts, A, b, t=t, return_info=True)
    assert info["alpha"] == 0.0 and (info["m"], info["s"], info["applications"]) == (0, 1, 0)
    Wd = tc.wide(T)
    for k in range(ts.size):
        want = np.exp(Wd(ts[k] * t) * Wd(c)) * b.astype(Wd)
        # 2 ulp: the rounding of the factor to T (eps / 2) and one product (real: eps / 2; complex: sqrt(5) eps / 2 in modulus)
        assert np.max(np.abs(W[:, k].astype(Wd) - want) / np.abs(want)) <= 2 * tc.eps_of(T), k
    assert np.array_equal(bits(W[:, int(np.argmin(ts))]), bits(b))


def test_max_matvecs_at_and_below_the_need(eu):
    n = 257
    A, b = tc.penta(n, np.float64), tc.vector(n, np.float64)
    t, ts = tc.t_for(A, 40.0), gc.rand13()
    op = eu.MIOperator(A)
    want, info = eu.expv_taylor_grid(ts, op, b, t=t, return_info=True)
    need = info["m"] * info["s"]
    W = np.full((n, ts.size), 7.0, order="F")
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_grid_(W, ts, op, b, t=t, max_matvecs=need - 1)
    msg = str(ei.value)
    assert ei.value.kind == "ArgumentError" and "alpha" in msg and "m* = %d" % info["m"] in msg and "s = %d" % info["s"] in msg, msg
    assert np.all(W == 7.0), "a refused call must leave W alone"
    eu.expv_taylor_grid_(W, ts, op, b, t=t, max_matvecs=need)
    assert np.array_equal(bits(W), bits(want))


def test_refusals(eu):
    n, q = 65, 4
    A, b = tc.penta(n, np.float64), tc.vector(n, np.float64)
    op = eu.MIOperator(A)
    r = np.array([0.5, 1.0, 0.0, 0.25])
    W = np.full((n, q), 7.0, order="F")
    buf = np.full(n * (q + 1), 7.0)

    def refused(what, **kw):
        args = dict(r=r, nt=q, b=b, W=W, ldw=n)
        args.update(kw)
        code, msg, _ = raw(eu, op, **args)
        assert code == 2 and what in msg, (code, msg)
        assert np.all(W == 7.0), "a refused call must leave W alone"
    refused("expv_taylor_grid", nt=-1)
    for bad in (-0.5, float("nan"), float("inf")):
        refused("expv_taylor_grid", r=np.array([0.5, bad, 1.0, 0.25]))
    refused("expv_taylor_grid: unknown layout", layout=2)
    refused("expv_taylor_grid: unknown loc", b_loc=2)
    refused("expv_taylor_grid: unknown loc", w_loc=-1)
    refused("expv_taylor_grid: leading dimension", ldw=n - 1)
    refused("expv_taylor_grid: leading dimension", ldw=q - 1, layout=1)
    refused("expv_taylor_grid: W overlaps b", b=buf[n - 1:2 * n - 1], W=buf, ldw=n)      # b begins on the last element of column 0
    refused("expv_taylor_grid: W overlaps b", b=buf[:n], W=buf, ldw=n)
    refused("expv_taylor: precision", precision=2)
    refused("expv_taylor: a complex t", t=(0.5, 0.25))
    assert np.all(buf == 7.0)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_grid([0.5, float("nan")], op, b)
    assert ei.value.kind == "ArgumentError"


def test_an_infinite_entry_in_the_operator_is_returned_not_raised(eu):
    """a matrix-free operator with an infinite coefficient and a finite bound: alpha is finite, the first term is not"""
    n = 129
    vals = list(C2_VALS)
    vals[1] = float("inf")
    op, sop = stencil(eu, n, vals)
    b = tc.vector(n, np.float64)
    ts = gc.rand13()
    W, info = eu.expv_taylor_grid(ts, op, b, t=1.0, opnorm=30.0, return_info=True)
    assert info["nonfinite_stage"] == 1 and not math.isfinite(info["normF"]) and info["s"] > 1
    for k in range(ts.size):
        if info["kind"][k] == 0:
            assert np.array_equal(bits(W[:, k]), bits(b))
        else:
            assert not np.all(np.isfinite(W[:, k])), "output %d of stage %d after a non-finite stage 0" % (k, info["stage"][k])
    assert info["applications"] < info["launches"]
    del sop


@pytest.mark.parametrize("mk,path", [(tc.random8, 1), (tc.powerlaw, 2)], ids=["fused", "update"])
def test_overflow_in_a_later_stage_leaves_the_earlier_outputs_right(eu, tables, mk, path):
    """Float32, |b| ~ 1e30 and a shift that grows F by 1e18 over the call: F overflows in a middle stage.  Status OK; every output of a
    later stage is non-finite; the outputs of the stages before it meet the bar; the context works afterwards."""
    n, T = 257, np.float32
    A0 = mk(n, T)
    base = tc.shift_norm(A0, 1.0)[1]
    t = 40.0 / base
    A = (A0 + sp.identity(n, format="csr") * (18.0 * math.log(10.0) / t)).astype(T).tocsr()
    b = (tc.vector(n, T) * T(1e30)).astype(T)
    ts = gc.lin40()
    mu, alpha, _ = tc.shift_norm(A, t)
    Wr, ir = gc.restated_grid(t, ts, A, b, T, alpha, tables[1], tc.TOL[1], mu)
    assert 2 <= ir["nonfinite_stage"] < ir["s"], ir
    op = eu.MIOperator(A)
    W, info = eu.expv_taylor_grid(ts, op, b, t=t, return_info=True)
    assert info["path"] == path and info["nonfinite_stage"] == ir["nonfinite_stage"] and not math.isfinite(info["normF"])
    truth = gc.truth_columns(A, b, t, ts)
    nf = info["nonfinite_stage"] - 1
    early = later = 0
    for k in range(ts.size):
        if info["stage"][k] > nf:
            later += 1
            assert not np.all(np.isfinite(W[:, k])), k
        elif info["stage"][k] < nf:
            early += 1
            e_r, e_d = tc.relmax(Wr[:, k], truth[:, k]), tc.relmax(W[:, k], truth[:, k])
            assert e_d <= BAR * max(e_r, tc.eps_of(T)), (k, e_d, e_r)
    assert early > 0 and later > 0
    good = tc.vector(n, T)
    check(eu, tables, mk.__name__ + " after overflow", A0, good, t, gc.rand13(), gc.truth_columns(A0, good, t, gc.rand13()), op=eu.MIOperator(A0))
