"""exponential!(A, ExpMethodHigham2005Base()) and LAPACK.gebal!('B', A) for a dense matrix on the device (expv_mi_expm_balanced,
expv_mi_gebal; csrc/dense_dev.hip), against the CPU sides of tests/balance_cases.py.

Balancing is checked EXACTLY: ilo, ihi and scale are equal to the numpy restatement's and the balanced matrix is its balanced matrix
bit for bit -- every operation on the data is a multiplication by a power of two, and every decision of the restatement is taken
with a relative margin of at least 1e-9, far above what the order of an fp64 sum can move.  The exponential is checked against the
exactly known truth of the inputs at the project's standing bars (1e-11 for the 64-bit types, 1e-4 for the 32-bit ones), and the
squarings against what the restatement predicts from the norm of the BALANCED matrix.  On the same badly scaled matrices the
unbalanced expv_mi_expm misses those bars: that assertion is the reason the entry exists.

SINGULAR cannot be provoked through either exponential entry with a finite matrix (the Pade denominator has no root inside the norm
bound that selects its order, and rounding does not produce an exactly zero pivot column).  The status path is therefore driven
through a host-side seam: a context created under EXPV_MI_DENSE_FORCE_SINGULAR=1 runs the whole computation and then answers as if
the LU had reported a zero pivot column -- what is checked is what the issue asks, the status and the untouched A.

expv_mi_expm's miss is asserted on the `scaled` inputs of n = 33, 130 and 545 wherever the same arithmetic on the CPU
(balance_cases.unbalanced_cpu_error) misses the bar by a factor 10 or does not stay finite; at n = 1100 that CPU prediction costs
tens of seconds per case (some 50 products of 1100 x 1100 complex matrices), so the size is left to the balanced checks."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import balance_cases as bc
from tests import dense_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARGUMENT_ERROR, SINGULAR = 0, 2, 4
UNBALANCED_SIZES = (33, 130, 545)
HOST, DEVICE = 0, 1
TYPES = list(bc.TYPES)
TOL = {"float64": 1e-11, "complex128": 1e-11, "float32": 1e-4, "complex64": 1e-4}
SIZES = [1, 2, 7, 33, 130, 545, 1100]      # 545: past one trip of the 512-thread workgroup; 1100: past 4096 workgroups of 256 element packs
FAMILIES = ["scaled12", "scaled20", "isolated03", "isolated50", "isolated46"]
PARITY_LOG = []


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module", autouse=True)
def _write_parity_log():
    yield
    if not PARITY_LOG:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "expm_balance_parity.txt"), "w") as f:
            f.write("# expv_mi_expm_balanced (and, where run, expv_mi_expm) against the exactly known exponential: relative Frobenius error\n")
            f.write("# written by tests/test_gpu_expm_balance.py (-m gpu); bars: 1e-11 (float64 / complex128), 1e-4 (float32 / complex64)\n")
            f.write("# %-11s %5s %-20s %4s %4s %5s %3s %6s  %-10s %s\n" % ("dtype", "n", "case", "ilo", "ihi", "order", "s", "sweeps", "balanced", "unbalanced (s)"))
            for row in PARITY_LOG:
                f.write("%-13s %5d %-20s %4d %4d %5d %3d %6d  %-10.3e %s\n" % row)
    except OSError:
        pass


def _code(eu, T):
    return eu.api._code(np.dtype(T))


def _case(tname, n, fam):
    if fam.startswith("scaled"):
        return bc.scaled(tname, n, int(fam[6:]))
    return bc.isolated(tname, n, int(fam[8]), int(fam[9]))


def _gebal(eu, ctx, A, lda=None, loc=DEVICE):
    """expv_mi_gebal on a copy of A inside an lda x n buffer whose extra rows hold NaN: (buffer afterwards, ilo, ihi, scale)"""
    n = A.shape[0]
    lda = n if lda is None else lda
    buf = np.full((max(lda, 1), n), np.nan, dtype=A.dtype, order="F")
    buf[:n, :] = A
    ilo, ihi = C.c_int64(-7), C.c_int64(-7)
    scale = np.full(n, np.nan)
    lib = eu.api.L.load()
    if loc == DEVICE:
        d = eu.DeviceArray.from_host(buf, ctx)
        st = lib.expv_mi_gebal(ctx._h, _code(eu, A.dtype), n, d.ptr, max(lda, 1), DEVICE, C.byref(ilo), C.byref(ihi), scale.ctypes.data)
        buf = d.to_host()
    else:
        st = lib.expv_mi_gebal(ctx._h, _code(eu, A.dtype), n, buf.ctypes.data, max(lda, 1), HOST, C.byref(ilo), C.byref(ihi), scale.ctypes.data)
    assert st == OK
    return buf, int(ilo.value), int(ihi.value), scale


def _assert_gebal(eu, ctx, case, lda=None, loc=DEVICE):
    A, g = case["A"], case["gebal"]
    n = A.shape[0]
    assert g["margin"] >= bc.MARGIN and g["sweeps"] < bc.BAL_MAX_SWEEPS
    buf, ilo, ihi, scale = _gebal(eu, ctx, A, lda, loc)
    assert (ilo, ihi) == (g["ilo"], g["ihi"])
    assert np.array_equal(scale, g["scale"])
    assert bc.same_bits(np.asfortranarray(buf[:n, :]), g["A_bal"])
    assert np.all(np.isnan(buf[n:, :])), "rows n..lda-1 were written"


# --------------------------------------------------------------------------------------------- balancing, exact
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tname", TYPES)
def test_gebal_is_the_restatement_bit_for_bit(eu, tname, n, fam):
    case = _case(tname, n, fam)
    ctx = eu.default_context()
    _assert_gebal(eu, ctx, case, lda=n + 3)
    if n <= 130:
        _assert_gebal(eu, ctx, case, lda=n + 1, loc=HOST)
        _assert_gebal(eu, ctx, case)


@pytest.mark.parametrize("tname", ["float32", "complex64"])
def test_the_norms_of_the_32_bit_types_are_summed_in_fp64(eu, tname):
    """r^2 = 64 + 2^-20 decides the second doubling of the first index: float32 sums lose the small square in any order"""
    case = bc.float32_sums_case(tname)
    wrong = bc.gebal_restated(case["A"], mutate="float32_sums")
    assert list(case["gebal"]["scale"]) == [4.0, 1.0, 64.0] and list(wrong["scale"]) == [2.0, 1.0, 32.0]
    ctx = eu.default_context()
    _assert_gebal(eu, ctx, case, lda=5)
    _assert_gebal(eu, ctx, case, loc=HOST)
    E, info = _expm(eu, ctx, case["A"], True)
    assert info[4:7] == [1, 3, case["gebal"]["sweeps"]] and dc.rel_err(E, case["truth"]) < TOL[tname]


@pytest.mark.parametrize("name", bc.DEGENERATE)
@pytest.mark.parametrize("tname", TYPES)
def test_gebal_on_degenerate_matrices(eu, tname, name):
    case = bc.degenerate(name, tname)
    g, n = case["gebal"], case["A"].shape[0]
    if name in ("permuted_triangular", "diagonal", "zero", "one", "negative_zeros"):
        assert (g["ilo"], g["ihi"], g["sweeps"]) == (1, 1, 0)                     # the l == 1 return
    if name == "zero_row_and_column":
        assert (g["ilo"], g["ihi"]) == (1, n - 1) and g["pos"][n - 1] == 4        # isolated by the row search, not skipped by the scaling loop
    ctx = eu.default_context()
    _assert_gebal(eu, ctx, case, lda=n + 2)
    _assert_gebal(eu, ctx, case, loc=HOST)


# --------------------------------------------------------------------------------------------- the exponential
def _expm(eu, ctx, A, balanced, lda=None, loc=DEVICE):
    n = A.shape[0]
    lda = n if lda is None else lda
    buf = np.full((max(lda, 1), n), np.nan, dtype=A.dtype, order="F")
    buf[:n, :] = A
    info = (C.c_int64 * 8)()
    lib = eu.api.L.load()
    fn = lib.expv_mi_expm_balanced if balanced else lib.expv_mi_expm
    if loc == DEVICE:
        d = eu.DeviceArray.from_host(buf, ctx)
        st = fn(ctx._h, _code(eu, A.dtype), n, d.ptr, max(lda, 1), DEVICE, info)
        buf = d.to_host()
    else:
        st = fn(ctx._h, _code(eu, A.dtype), n, buf.ctypes.data, max(lda, 1), HOST, info)
    assert st == OK
    assert np.all(np.isnan(buf[n:, :]))
    return np.asfortranarray(buf[:n, :]), list(info)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tname", TYPES)
def test_balanced_exponential_meets_the_bars_the_unbalanced_one_misses(eu, tname, n, fam):
    case = _case(tname, n, fam)
    A, g = case["A"], case["gebal"]
    ctx = eu.default_context()
    E, info = _expm(eu, ctx, A, True, lda=n + 3)
    err = dc.rel_err(E, case["truth"])
    unb = ""
    predicted = bc.unbalanced_cpu_error(tname, n, int(fam[6:])) if fam.startswith("scaled") and n in UNBALANCED_SIZES else 0.0
    if not predicted < 10 * TOL[tname]:
        with np.errstate(all="ignore"):
            U, uinfo = _expm(eu, ctx, A, False)
            uerr = dc.rel_err(U, case["truth"])
        unb = "%.3e (%d; cpu %.1e)" % (uerr, uinfo[1], predicted)
    print("%s n=%d %s ilo=%d ihi=%d order=%d s=%d sweeps=%d balancing=%dus of %dus err=%.3e unbalanced=%s"
          % (tname, n, fam, info[4], info[5], info[0], info[1], info[6], info[7], info[3], err, unb or "-"))
    PARITY_LOG.append((tname, n, fam, info[4], info[5], info[0], info[1], info[6], err, unb or "-"))
    assert (info[4], info[5], info[6]) == (g["ilo"], g["ihi"], g["sweeps"])
    assert (info[0], info[1]) == (g["order"], g["s"])            # from the norm AFTER balancing
    assert 0 <= info[7] <= info[3]
    assert err < TOL[tname]
    if unb:
        assert uinfo[1] >= 14                                    # the unbalanced norm asks for 14 .. 36 squarings here
        assert not uerr < TOL[tname], "expv_mi_expm meets the bar on a matrix scaled over 2^%s: the test has lost its reason" % fam[6:]


@pytest.mark.parametrize("name", bc.DEGENERATE)
@pytest.mark.parametrize("tname", TYPES)
def test_balanced_exponential_on_degenerate_matrices(eu, tname, name):
    case = bc.degenerate(name, tname)
    g = case["gebal"]
    E, info = _expm(eu, eu.default_context(), case["A"], True)
    assert (info[4], info[5], info[6]) == (g["ilo"], g["ihi"], g["sweeps"]) and (info[0], info[1]) == (g["order"], g["s"])
    assert dc.rel_err(E, case["truth"]) < TOL[tname]
    if name == "zero":
        assert np.array_equal(E, np.eye(5, dtype=tname))


# --------------------------------------------------------------------------------------------- nothing to balance: expv_mi_expm's bits
def _equal_magnitude_class(tname, n, seed):
    """entries with magnitude in [1, 2) / n: every row and column norm within a factor 2 of every other -- nothing to scale"""
    T = np.dtype(tname)
    rng = np.random.default_rng(seed)
    M = rng.uniform(1.0, 1.4, (n, n)) * rng.choice([-1.0, 1.0], (n, n))
    if T.kind == "c":
        M = M * np.exp(1j * rng.uniform(0, 2 * np.pi, (n, n)))
    return np.asfortranarray((M * (3.0 / n)).astype(T))


@pytest.mark.parametrize("tname", TYPES)
def test_an_already_balanced_matrix_gives_the_unbalanced_bits(eu, tname):
    ctx = eu.default_context()
    inputs = [_equal_magnitude_class(tname, n, 5 + n) for n in (33, 130)] + [dc.skew_case(tname, 130, 6, 5.0, with_gap=False)["A"]]
    for A in inputs:
        n = A.shape[0]
        g = bc.gebal_restated(A)
        assert (g["ilo"], g["ihi"]) == (1, n) and np.all(g["scale"] == 1.0) and g["margin"] >= bc.MARGIN
        B, binfo = _expm(eu, ctx, A, True)
        U, uinfo = _expm(eu, ctx, A, False)
        assert np.array_equal(B, U) and binfo[:3] == uinfo[:3]
        assert (binfo[4], binfo[5], binfo[6]) == (1, n, 1)
        buf, ilo, ihi, scale = _gebal(eu, ctx, A)
        assert (ilo, ihi) == (1, n) and np.all(scale == 1.0) and bc.same_bits(buf, np.asfortranarray(A))


# --------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("tname", TYPES)
def test_nonfinite_input_and_empty_matrix(eu, tname):
    lib, ctx = eu.api.L.load(), eu.default_context()
    A = bc.scaled(tname, 33, 12)["A"]
    for bad in (np.nan, np.inf):
        B = np.array(A, order="F")
        B[7, 20] = bad
        keep = B.copy()
        with pytest.raises(eu.ExpvMIError, match="matrix contains Infs or NaNs") as ei:
            eu.exponential_(B, balance=True)
        assert ei.value.code == ARGUMENT_ERROR
        assert np.array_equal(B, keep, equal_nan=True)
        d = eu.DeviceArray.from_host(B, ctx)
        assert lib.expv_mi_expm_balanced(ctx._h, _code(eu, tname), 33, d.ptr, 33, DEVICE, None) == ARGUMENT_ERROR
        assert np.array_equal(d.to_host(), keep, equal_nan=True)
        assert lib.expv_mi_gebal(ctx._h, _code(eu, tname), 33, d.ptr, 33, DEVICE, None, None, None) == ARGUMENT_ERROR
        assert np.array_equal(d.to_host(), keep, equal_nan=True)
    assert lib.expv_mi_expm_balanced(ctx._h, _code(eu, tname), 0, None, 0, DEVICE, None) == OK
    ilo, ihi = C.c_int64(-7), C.c_int64(-7)
    assert lib.expv_mi_gebal(ctx._h, _code(eu, tname), 0, None, 0, DEVICE, C.byref(ilo), C.byref(ihi), None) == OK
    assert (ilo.value, ihi.value) == (1, 0)
    E = eu.exponential(np.zeros((0, 0), dtype=tname), balance=True)
    assert E.shape == (0, 0)
    assert eu.balance_(np.zeros((0, 0), dtype=tname))[:2] == (1, 0)


@pytest.mark.parametrize("tname", TYPES)
def test_a_singular_denominator_answers_singular_with_a_untouched(eu, tname):
    """the status path through the seam (see the module docstring): both entries, DEVICE and HOST, lda > n"""
    lib = eu.api.L.load()
    old = os.environ.get("EXPV_MI_DENSE_FORCE_SINGULAR")
    os.environ["EXPV_MI_DENSE_FORCE_SINGULAR"] = "1"
    try:
        ctx = eu.Context()
    finally:
        if old is None:
            os.environ.pop("EXPV_MI_DENSE_FORCE_SINGULAR", None)
        else:
            os.environ["EXPV_MI_DENSE_FORCE_SINGULAR"] = old
    A = bc.isolated(tname, 33, 4, 6)["A"]
    buf = np.full((36, 33), np.nan, dtype=tname, order="F")
    buf[:33, :] = A
    for fn in (lib.expv_mi_expm_balanced, lib.expv_mi_expm):
        info = (C.c_int64 * 8)()
        d = eu.DeviceArray.from_host(buf, ctx)
        assert fn(ctx._h, _code(eu, tname), 33, d.ptr, 36, DEVICE, info) == SINGULAR
        assert np.array_equal(d.to_host(), buf, equal_nan=True)
        h = buf.copy(order="F")
        assert fn(ctx._h, _code(eu, tname), 33, h.ctypes.data, 36, HOST, info) == SINGULAR
        assert np.array_equal(h, buf, equal_nan=True)
    B = np.array(A, order="F")
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.exponential_(B, balance=True, ctx=ctx)
    assert ei.value.code == SINGULAR and np.array_equal(B, A)
    # the same matrix through an ordinary context: nothing is singular about it
    E = eu.exponential(A, balance=True)
    assert dc.rel_err(E, bc.isolated(tname, 33, 4, 6)["truth"]) < TOL[tname]
    # balancing itself has no such status
    assert lib.expv_mi_gebal(ctx._h, _code(eu, tname), 33, eu.DeviceArray.from_host(buf, ctx).ptr, 36, DEVICE, None, None, None) == OK


# --------------------------------------------------------------------------------------------- workspace and ordering
def test_a_workspace_reused_after_a_larger_call_reproduces_bits(eu):
    ctx = eu.Context()
    small, big, other = bc.isolated("float64", 33, 4, 6)["A"], bc.scaled("complex64", 545, 20)["A"], bc.scaled("float32", 130, 12)["A"]
    first, finfo = _expm(eu, ctx, small, True)
    g1 = _gebal(eu, ctx, small)
    _expm(eu, ctx, big, True)
    _expm(eu, ctx, other, False)
    again, ainfo = _expm(eu, ctx, small, True)
    g2 = _gebal(eu, ctx, small)
    assert np.array_equal(first, again) and finfo[:3] == ainfo[:3] and finfo[4:7] == ainfo[4:7]
    assert bc.same_bits(g1[0], g2[0]) and g1[1:3] == g2[1:3] and np.array_equal(g1[3], g2[3])


def test_back_to_back_stream_ordered_calls_reproduce_the_synchronous_bits(eu):
    lib = eu.api.L.load()
    c1, c2 = bc.isolated("float64", 130, 4, 6), bc.scaled("float64", 33, 20)
    A1, A2 = c1["A"], c2["A"]
    sync_ctx = eu.Context()
    want1, _ = _expm(eu, sync_ctx, A1, True)
    want2, _ = _expm(eu, sync_ctx, A2, True)
    wantg = _gebal(eu, sync_ctx, A1)[0]
    ctx = eu.Context(async_outputs=True)
    d1, d2, d3 = (eu.DeviceArray.from_host(np.array(M, order="F"), ctx) for M in (A1, A2, A1))
    i1, i2 = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    code = _code(eu, np.float64)
    assert lib.expv_mi_expm_balanced(ctx._h, code, 130, d1.ptr, 130, DEVICE, i1) == OK
    assert lib.expv_mi_expm_balanced(ctx._h, code, 33, d2.ptr, 33, DEVICE, i2) == OK
    assert lib.expv_mi_gebal(ctx._h, code, 130, d3.ptr, 130, DEVICE, None, None, None) == OK
    ctx.sync()
    assert np.array_equal(d1.to_host(), want1) and np.array_equal(d2.to_host(), want2) and bc.same_bits(d3.to_host(), wantg)
    assert (i1[4], i1[5]) == (c1["gebal"]["ilo"], c1["gebal"]["ihi"]) == (5, 124) and (i2[4], i2[5]) == (1, 33)


# --------------------------------------------------------------------------------------------- Python wrappers
@pytest.mark.parametrize("tname", TYPES)
def test_python_wrappers_on_torch_and_numpy(eu, tname):
    import torch
    case = bc.isolated(tname, 33, 4, 6)
    A, g = case["A"], case["gebal"]
    # numpy, in place and copying, with the info dict
    a = np.array(A, order="F")
    out, info = eu.exponential_(a, balance=True, return_info=True)
    assert out is a and dc.rel_err(a, case["truth"]) < TOL[tname]
    assert (info["ilo"], info["ihi"], info["sweeps"], info["squarings"]) == (g["ilo"], g["ihi"], g["sweeps"], g["s"])
    assert np.array_equal(eu.exponential(A, balance=True), a) and np.array_equal(A, case["A"])
    b = np.array(A, order="F")
    ilo, ihi, scale = eu.balance_(b)
    assert (ilo, ihi) == (g["ilo"], g["ihi"]) and np.array_equal(scale, g["scale"]) and bc.same_bits(b, g["A_bal"])
    c = np.array(A, order="C")                                   # row-major numpy: balanced as the matrix it is, through a copy
    eu.balance_(c)
    assert np.array_equal(c, g["A_bal"])
    # torch: column-major storage in place, row-major through the transpose
    t_col = torch.from_numpy(np.array(A.T, order="C")).cuda().t()
    assert t_col.stride(0) == 1
    ilo, ihi, scale = eu.balance_(t_col)
    assert (ilo, ihi) == (g["ilo"], g["ihi"]) and np.array_equal(scale, g["scale"]) and np.array_equal(t_col.cpu().numpy(), g["A_bal"])
    t_row = torch.from_numpy(np.array(A, order="C")).cuda()
    assert t_row.is_contiguous()
    assert eu.balance_(t_row)[:2] == (g["ilo"], g["ihi"]) and np.array_equal(t_row.cpu().numpy(), g["A_bal"])
    e_col = eu.exponential_(torch.from_numpy(np.array(A.T, order="C")).cuda().t(), balance=True)
    assert np.array_equal(e_col.cpu().numpy(), a)
    e_row = eu.exponential_(torch.from_numpy(np.array(A, order="C")).cuda(), balance=True)       # exp(A') = exp(A)'
    assert dc.rel_err(e_row.cpu().numpy(), case["truth"]) < TOL[tname]
    da = eu.DeviceArray.from_host(A, eu.default_context())
    assert eu.exponential_(da, balance=True) is da and np.array_equal(da.to_host(), a)
    # the default is the unbalanced entry, unchanged
    plain, pinfo = eu.exponential(A, return_info=True)
    assert set(pinfo) == {"order", "squarings", "row_exchanges", "microseconds"}
