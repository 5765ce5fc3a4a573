"""The block 1-norm estimator on the device (expv_mi_op_norm_power, MIOperator.norm_power) against its numpy restatement
(tests/normest_cases.py) and the exact norms of dense powers.

Bar: |est_dev - est_restated| <= 8 p r eps_T || |B|^p ||, r the longest row of B = A - sigma I -- the device and the restatement run
the same algorithm on the same signs and differ in the summation order inside a row (p applications, r terms each), taken against
the norm of the entrywise absolute operator.  The trace (iterations, exit, best index, resamples, blocking reads) is the same.  The
measured differences go to profiles/normest_parity.txt."""
import math
import os
import warnings

import numpy as np
import pytest

from tests import normest_cases as nc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (2, 5, 9)
_lines, _ops = [], {}


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    if not _lines:
        return
    path = os.path.join(ROOT, "profiles", "normest_parity.txt")
    try:
        with open(path, "w") as f:
            f.write("# norm_power against the numpy restatement: |est_dev - est_restated| and the bar 8 p r eps || |B|^p ||; ratio = est_dev / exact norm\n")
            f.write("%-20s %-10s %2s %4s %22s %10s %10s %9s %4s %4s %5s\n" % ("case", "dtype", "p", "norm", "est_dev", "diff", "bar", "ratio", "exit", "it", "reads"))
            f.write("\n".join(_lines) + "\n")
    except OSError as e:      # (a read-only checkout: the tests have passed, the table is what is lost -- say so)
        warnings.warn("profiles/normest_parity.txt was not written: %s" % e)


def operators(eu, name):
    """(op, adj) of a case, made once; the shuffled band on a context that always keeps the bandwidth-reducing ordering"""
    if name not in _ops:
        A, _ = nc.case(name)
        if name == "shuffled_band_2000":
            ctx = eu.Context()
            ctx.set_option("reorder", 2)
            op = eu.MIOperator(A, ctx)
            assert op.reorder_info["reordered"]
        else:
            op = eu.MIOperator(A)
        _ops[name] = (op, op.adjoint())
    return _ops[name]


def bar_of(A, p, absnorm):
    return 8 * p * nc.longest_row(A) * float(np.finfo(A.dtype).eps) * absnorm


def bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("which", [0, 1], ids=["inf", "one"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_norm_power_against_the_restatement(eu, name, p, which):
    A, sigma = nc.case(name)
    op, adj = operators(eu, name)
    ex = nc.exact_norms(name, A, sigma)[p]
    est_r, tr = nc.restated(A, p, sigma, which)
    est, info = op.norm_power(p, np.inf if which == 0 else 1, sigma, None if name == "hermitian_777" else adj, return_info=True)
    bar = bar_of(A, p, ex[2 + which])
    _lines.append("%-20s %-10s %2d %4s %22.15e %10.2e %10.2e %9.6f %4d %4d %5d" % (name, A.dtype.name, p, "inf" if which == 0 else "1", est, abs(est - est_r), bar,
                                                                               est / ex[which], info["exit"], info["iterations"], info["host_reads"]))
    print("[normest]", _lines[-1])
    assert (info["iterations"], info["exit"], info["index"], info["resamples"]) == (tr["iterations"], tr["exit"], tr["index"], tr["resamples"]), (info, tr)
    assert info["applications"] == tr["applications"] and info["host_reads"] == tr["reads"] <= 2 * info["iterations"] + info["resamples"], (info, tr)
    assert info["temporary_adjoint"] == 0
    assert abs(est - est_r) <= bar, (est, est_r, bar)
    assert est <= ex[which] + bar * min(1.0, ex[which]), (est, ex[which], bar)
    assert bits(op.norm_power(p, np.inf if which == 0 else 1, sigma, None if name == "hermitian_777" else adj)) == bits(est), "two calls, other bits"


@pytest.mark.parametrize("name", ["bt200", "schroedinger_c128", "dense300", "powerlaw_1000"])
def test_temporary_adjoint_gives_the_same_bits(eu, name):
    A, sigma = nc.case(name)
    op, adj = operators(eu, name)
    for which in (0, 1):
        e1, i1 = op.norm_power(5, np.inf if which == 0 else 1, sigma, adj, return_info=True)
        e2, i2 = op.norm_power(5, np.inf if which == 0 else 1, sigma, None, return_info=True)
        assert bits(e1) == bits(e2)
        assert i1["temporary_adjoint"] == 0 and i2["temporary_adjoint"] == 1 and i2["adjoint_us"] > 0
        assert {k: v for k, v in i1.items() if k not in ("temporary_adjoint", "adjoint_us")} == {k: v for k, v in i2.items() if k not in ("temporary_adjoint", "adjoint_us")}


def test_hermitian_operator_is_its_own_adjoint(eu):
    A, sigma = nc.case("hermitian_777")
    op, adj = operators(eu, "hermitian_777")
    assert op.ishermitian
    e1, i1 = op.norm_power(5, np.inf, sigma, None, return_info=True)
    e2, i2 = op.norm_power(5, np.inf, sigma, adj, return_info=True)
    assert i1["temporary_adjoint"] == 0 and i1["adjoint_us"] == 0
    assert abs(e1 - e2) <= bar_of(A, 5, nc.exact_norms("hermitian_777", A, sigma)[5][2])


@pytest.mark.parametrize("p", PS)
def test_reordered_operator_against_its_unpermuted_twin(eu, p):
    A, sigma = nc.case("shuffled_band_2000")
    op, adj = operators(eu, "shuffled_band_2000")
    ex = nc.exact_norms("shuffled_band_2000", A, sigma)[p]
    # the twin: the same operator stored in the caller's numbering.  Signs are drawn on natural rows and indices are reported in the
    # natural numbering, so the whole trace is the same and the estimates differ by rounding
    plain = eu.Context()
    plain.set_option("reorder", 0)
    p_op = eu.MIOperator(A, plain)
    assert not p_op.reorder_info["reordered"]
    p_adj = p_op.adjoint()
    for which in (0, 1):
        e, i = op.norm_power(p, np.inf if which == 0 else 1, sigma, adj, return_info=True)
        ep, ip = p_op.norm_power(p, np.inf if which == 0 else 1, sigma, p_adj, return_info=True)
        assert abs(e - ep) <= bar_of(A, p, ex[2 + which]) and i == ip, (i, ip)


@pytest.mark.parametrize("p", PS)
def test_reordered_operator_without_a_fused_form(eu, p):
    """irregular rows kept in the bandwidth-reducing ordering: mul! + update behind a gather into the stored ordering and back"""
    A, sigma = nc.case("powerlaw_1000")
    ctx = eu.Context()
    ctx.set_option("reorder", 2)
    op = eu.MIOperator(A, ctx)
    assert op.reorder_info["reordered"]
    adj = op.adjoint()
    p_op, p_adj = operators(eu, "powerlaw_1000")
    ex = nc.exact_norms("powerlaw_1000", A, sigma)[p]
    for which in (0, 1):
        e, i = op.norm_power(p, np.inf if which == 0 else 1, sigma, adj, return_info=True)
        ep, ip = p_op.norm_power(p, np.inf if which == 0 else 1, sigma, p_adj, return_info=True)
        er, tr = nc.restated(A, p, sigma, which)
        assert abs(e - er) <= bar_of(A, p, ex[2 + which]) and abs(e - ep) <= bar_of(A, p, ex[2 + which])
        assert i == ip and (i["iterations"], i["exit"], i["index"]) == (tr["iterations"], tr["exit"], tr["index"]), (i, ip, tr)


def test_scaling_by_powers_of_two_keeps_the_mantissa(eu):
    """Float32, p = 9: the ninth power of 2^20 A overflows Float32 and that of 2^-20 A vanishes in it; the estimate moves by 2^(+-180)"""
    A, sigma = nc.case("bt1537_f32")
    op, adj = operators(eu, "bt1537_f32")
    e0, i0 = op.norm_power(9, np.inf, sigma, adj, return_info=True)
    assert e0 * 2.0 ** 180 > float(np.finfo(np.float32).max) and e0 * 2.0 ** -180 < float(np.finfo(np.float32).tiny)
    for k in (20, -20):
        Ak = (A * np.float32(2.0 ** k)).astype(np.float32).tocsr()
        opk = eu.MIOperator(Ak)
        e, i = opk.norm_power(9, np.inf, sigma * 2.0 ** k, opk.adjoint(), return_info=True)
        assert math.isfinite(e) and e > 0
        assert math.frexp(e)[0] == math.frexp(e0)[0], (e, e0)
        assert math.frexp(e)[1] - math.frexp(e0)[1] == 9 * k
        assert i == i0


@pytest.mark.parametrize("name", ["bt200", "schroedinger_c128", "dense300"])
def test_first_power_in_the_infinity_norm_is_exact(eu, name):
    A, sigma = nc.case(name)
    op, _ = operators(eu, name)
    if np.finfo(A.dtype).eps > 1e-10:      # sigma as the kernels of a 32-bit operator take it
        sigma = complex(np.complex64(sigma)) if A.dtype.kind == "c" else float(np.float32(sigma))
    B = nc.shifted(A, sigma)
    want = float(np.abs(B).sum(axis=1).max())
    est, info = op.norm_power(1, np.inf, sigma, None, return_info=True)
    assert abs(est - want) <= 4 * nc.longest_row(A) * float(np.finfo(np.float64).eps) * want
    assert info["exit"] == nc.EXIT_EXACT and info["temporary_adjoint"] == 0 and info["applications"] == 0


@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("n", [1, 2])
def test_fewer_than_three_rows_are_exact(eu, n, T):
    A = np.asfortranarray(np.array([[1.5, -2.0], [0.25, 3.0]])[:n, :n].astype(T))
    if np.dtype(T).kind == "c":
        A = np.asfortranarray((A * (0.6 + 0.8j)).astype(T))
    op = eu.MIOperator(A)
    for p in (1, 3):
        M = np.linalg.matrix_power(A.astype(np.complex128) - 0.5 * np.eye(n), p)
        for which in (0, 1):
            est, info = op.norm_power(p, np.inf if which == 0 else 1, 0.5, return_info=True)
            assert info["exit"] == nc.EXIT_EXACT
            assert est == pytest.approx(np.abs(M).sum(axis=1 - which).max(), rel=64 * float(np.finfo(T).eps))


def test_argument_errors(eu):
    A, sigma = nc.case("bt200")
    op, adj = operators(eu, "bt200")
    for p in (0, 17, -3):
        with pytest.raises(eu.ExpvMIError, match="outside 1 .. 16"):
            op.norm_power(p, np.inf, sigma, adj)
    with pytest.raises(eu.ExpvMIError, match="which"):
        op.norm_power(2, 2, sigma, adj)
    other = eu.Context()
    with pytest.raises(eu.ExpvMIError, match="another context"):
        op.norm_power(2, np.inf, sigma, eu.MIOperator(A, other).adjoint())
    with pytest.raises(eu.ExpvMIError, match="dtype or n"):
        op.norm_power(2, np.inf, sigma, eu.MIOperator(A.astype(np.float32)).adjoint())
    with pytest.raises(eu.ExpvMIError, match="dtype or n"):
        op.norm_power(2, np.inf, sigma, eu.MIOperator(nc.block_triangular(100)).adjoint())
    with pytest.raises(eu.ExpvMIError, match="complex shift"):
        op.norm_power(2, np.inf, 1.0 + 1.0j, adj)
    n = A.shape[0]
    Ad = A.toarray()
    mf = eu.MIOperator(None, matvec=lambda x: Ad @ x, shape=(n, n), dtype=np.float64, ishermitian=False)
    for a in (None, adj):
        with pytest.raises(eu.ExpvMIError, match="matrix-free") as ei:
            mf.norm_power(2, np.inf, sigma, a)
        assert ei.value.kind == "Unsupported"
    with pytest.raises(eu.ExpvMIError, match="matrix-free") as ei:
        op.norm_power(2, np.inf, sigma, mf)
    assert ei.value.kind == "Unsupported"
