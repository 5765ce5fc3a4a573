"""The norm estimator and the whole Taylor parameter search, as far as a machine without a GPU can check them: the host-only exports
against their Python restatements, and the conditions the committed cases of tests/normest_cases.py have to meet so that the GPU
tests can hold the device to the restatement's trace.

Conditions on every case, p = 2, 5, 9 (the exact ||B^p|| from dense powers in 64-bit arithmetic):
  - restated est <= exact (1 + 1e-12) in both norms: an estimate is the 1-norm of a vector M x with |x|_1 = 1.  The two Float32 cases
    hit the exact norm and carry Float32 roundings of 1e-8 .. 1e-7 of it, which no 1e-12 can hold: for them the bound is asserted
    on the restatement run in fp64 (same trace, asserted below), and the Float32 run stays within the row-summation bar
    8 p r eps || |B|^p || of it -- the bar the device is held to;
  - restated est >= 0.9 exact in both norms (measured: >= 0.907; block-triangular >= 0.946);
  - the same trace (iterations, visited indices, best index, exit) in the element type and in wider arithmetic (fp64 for the
    32-bit cases, longdouble for the 64-bit ones): no decision of the loop hangs on a rounding."""
import math
import os

import numpy as np
import pytest

from tests import expv_taylor_cases as tc
from tests import normest_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (2, 5, 9)


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, nc.M_MAX + 1)] for p in (0, 1)}


# ---- signs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,col,attempt", [(0, 0, 0), (1, 1, 0), (2, 1, 0), (257, 0, 3), (3074, 1, 0), (3074, 1, 1), (100000, 1, 7), (1000, 0, 2 ** 32 - 1)])
def test_signs_are_the_librarys(eu, n, col, attempt):
    got = eu.host_normest_signs(n, col, attempt)
    assert got.dtype == np.int8 and got.shape == (n,)
    assert np.array_equal(got, nc.sign_hash(n, col, attempt))
    if n >= 257:
        assert set(np.unique(got)) == {-1, 1} and abs(int(got.astype(np.int64).sum())) < 5 * math.sqrt(n)


def test_signs_differ_between_columns_and_draws(eu):
    a, b, c = eu.host_normest_signs(4096, 1, 0), eu.host_normest_signs(4096, 1, 1), eu.host_normest_signs(4096, 0, 0)
    for x, y in ((a, b), (a, c), (b, c)):
        assert 1500 < np.count_nonzero(x == y) < 2600


def test_signs_argument_errors(eu):
    for args in ((-1, 0, 0), (4, -1, 0), (4, 0, -1), (4, 0, 2 ** 32)):
        with pytest.raises(eu.ExpvMIError):
            eu.host_normest_signs(*args)


# ---- the parameter search -------------------------------------------------------------------------------------------------------
def _d_sequences(alpha1, rng):
    """decreasing d_2 .. d_9 below alpha1: geometric decays, a plateau, random decreasing, and all equal to alpha1"""
    yield [alpha1] * 8
    for q in (0.9, 0.5, 0.1):
        yield [alpha1 * q ** (i + 1) for i in range(8)]
    yield [alpha1 * 0.3] * 4 + [alpha1 * 0.01] * 4
    yield sorted((alpha1 * rng.random(8)).tolist(), reverse=True)


@pytest.mark.parametrize("precision", [0, 1])
def test_params_power_against_brute_force(eu, tables, precision):
    rng = np.random.default_rng(3)
    th = tables[precision]
    n = 0
    for alpha1 in np.logspace(-3, 5, 49):
        for d in _d_sequences(float(alpha1), rng):
            assert eu.host_taylor_params_power(alpha1, d, precision) == nc.params_power(float(alpha1), d, th), (alpha1, d)
            n += 1
    assert n == 49 * 6


@pytest.mark.parametrize("precision", [0, 1])
def test_params_power_never_costs_more_than_the_first_branch(eu, precision):
    rng = np.random.default_rng(4)
    for alpha1 in np.logspace(-3, 5, 33):
        m1, s1 = eu.host_taylor_params(alpha1, precision)
        for d in _d_sequences(float(alpha1), rng):
            m, s, _ = eu.host_taylor_params_power(alpha1, d, precision)
            assert m * s <= m1 * s1, (alpha1, d, (m, s), (m1, s1))


@pytest.mark.parametrize("precision", [0, 1])
def test_params_power_edges(eu, tables, precision):
    th = tables[precision]
    cheap = 4 * th[54] * 8 * 11 / 55
    zeros = [0.0] * 8
    assert eu.host_taylor_params_power(0.0, zeros, precision) == (0, 1, 0)
    # at the threshold: the first branch, whatever d holds; one ulp past it: the second
    assert eu.host_taylor_params_power(cheap, zeros, precision) == eu.host_taylor_params(cheap, precision) + (0,)
    past = float(np.nextafter(cheap, np.inf))
    assert eu.host_taylor_params_power(past, zeros, precision) == (1, 1, 2)
    assert eu.host_taylor_params_power(past, [past] * 8, precision) == nc.params_power(past, [past] * 8, th)
    assert eu.host_taylor_params_power(past, [past] * 8, precision)[2] >= 2
    assert eu.host_taylor_params_power(1e4, zeros, precision) == (1, 1, 2)
    # ties: alpha_p = theta_m exactly costs m for several (p, m); the smallest (cost, m) wins, the first p that reaches it
    for m in (5, 11, 19, 29, 41):
        d = [th[m - 1]] * 8
        got = eu.host_taylor_params_power(1e3, d, precision)
        assert got == nc.params_power(1e3, d, th) and got[0] * got[1] <= m
    # only d_p and d_{p+1} of the winner matter
    d = [50.0, 20.0, 1.0, 1.0, 30.0, 30.0, 30.0, 30.0]
    assert eu.host_taylor_params_power(1e3, d, precision) == nc.params_power(1e3, d, th)
    assert eu.host_taylor_params_power(1e3, d, precision)[2] == 4
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(eu.ExpvMIError):
            eu.host_taylor_params_power(bad, zeros, precision)
        with pytest.raises(eu.ExpvMIError):
            eu.host_taylor_params_power(1e3, [bad] + [1.0] * 7, precision)
    with pytest.raises(eu.ExpvMIError):
        eu.host_taylor_params_power(1.0, zeros, 2)
    with pytest.raises(eu.DimensionMismatch):
        eu.host_taylor_params_power(1.0, [1.0] * 7, precision)


# ---- the committed cases ------------------------------------------------------------------------------------------------------------
def _trace_key(tr):
    return tr["iterations"], tr["exit"], tr["index"], tuple(tr["hist"]), tr["resamples"]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_case_conditions(name, p):
    A, sigma = nc.case(name)
    ex = nc.exact_norms(name, A, sigma)[p]
    for which in (0, 1):
        est, tr = nc.restated(A, p, sigma, which)
        print("[normest] %-20s p=%d which=%d est/exact = %.6f exit %d iterations %d resamples %d" % (name, p, which, est / ex[which], tr["exit"], tr["iterations"], tr["resamples"]))
        est_w, tr_w = nc.restated(A, p, sigma, which, arith=nc.wider(A.dtype))
        assert (est if np.finfo(A.dtype).eps < 1e-10 else est_w) <= ex[which] * (1 + 1e-12), (name, p, which, est, est_w, ex[which])
        assert est >= 0.9 * ex[which], (name, p, which, est / ex[which])
        assert tr["exit"] == nc.EXITS[name], (name, p, which, tr)
        assert tr["reads"] == 2 * tr["iterations"] - (1 if tr["exit"] in (nc.EXIT_NO_GROWTH, nc.EXIT_ITMAX, nc.EXIT_PARALLEL) else 0) + tr["resamples"]
        assert _trace_key(tr) == _trace_key(tr_w), (name, p, which, tr, tr_w)
        assert abs(est - est_w) <= 8 * p * nc.longest_row(A) * np.finfo(A.dtype).eps * ex[2 + which]


def test_exits_covered():
    assert {nc.EXIT_NO_GROWTH, nc.EXIT_HMAX_IS_BEST, nc.EXIT_PARALLEL} <= set(nc.EXITS.values())
    assert set(nc.EXITS) == set(nc.CASE_NAMES)


@pytest.mark.parametrize("n", [1, 2])
def test_restatement_is_exact_below_three_rows(n):
    A = np.asfortranarray(np.array([[1.5, -2.0], [0.25, 3.0]])[:n, :n])
    for p in (1, 3):
        M = np.linalg.matrix_power(A - 0.5 * np.eye(n), p)
        for which in (0, 1):
            est, tr = nc.restated(A, p, 0.5, which)
            assert tr["exit"] == nc.EXIT_EXACT and est == pytest.approx(np.abs(M).sum(axis=1 - which).max(), rel=1e-14)


def test_restatement_scales_by_exact_powers_of_two():
    """est of 2^k A is 2^(kp) est of A with the same mantissa, far outside the range of Float32"""
    A, sigma = nc.case("bt1537_f32")
    e0, tr0 = nc.restated(A, 9, sigma, 0)
    for k in (20, -20):
        s = np.float32(2.0 ** k)
        e, tr = nc.restated((A * s).astype(np.float32).tocsr(), 9, sigma * 2.0 ** k, 0)
        assert math.frexp(e)[0] == math.frexp(e0)[0] and math.frexp(e)[1] - math.frexp(e0)[1] == 9 * k
        assert _trace_key(tr) == _trace_key(tr0)
    assert e0 * 2.0 ** 180 > float(np.finfo(np.float32).max)


def test_headline_numbers(eu, tables):
    """the block-triangular case of order 1537, t = 1, the 2^-53 table: 46 operator applications planned against 16 665"""
    A, mu = nc.case("bt1537")
    _, alpha1, _ = tc.shift_norm(A, 1.0)
    d = nc.restated_d(A, 1.0, mu)
    assert all(d[i] >= d[i + 1] for i in range(7)) and d[0] <= alpha1
    m, s, p_used = eu.host_taylor_params_power(alpha1, d, 0)
    assert (m, s, p_used) == nc.params_power(alpha1, d, tables[0])
    m1, s1 = eu.host_taylor_params(alpha1, 0)
    print("[normest] bt1537: alpha1 = %.1f first branch (%d, %d) = %d, with power norms (%d, %d) p = %d" % (alpha1, m1, s1, m1 * s1, m, s, p_used))
    assert m * s <= 60
    assert m1 * s1 >= 10 ** 4


def test_the_refined_series_is_as_accurate_at_order_200(eu, tables):
    A, mu = nc.case("bt200")
    _, alpha1, _ = tc.shift_norm(A, 1.0)
    m, s, _ = eu.host_taylor_params_power(alpha1, nc.restated_d(A, 1.0, mu), 0)
    m1, s1 = eu.host_taylor_params(alpha1, 0)
    b = tc.vector(A.shape[0], np.float64)
    import scipy.linalg as sl
    truth = sl.expm(A.toarray()) @ b
    F, apps = nc.restated_series(1.0, A, b, m, s, mu, tc.TOL[0])
    F1, apps1 = nc.restated_series(1.0, A, b, m1, s1, mu, tc.TOL[0])
    print("[normest] bt200: %d applications, error %.2e; first branch %d applications, error %.2e" % (apps, tc.relmax(F, truth), apps1, tc.relmax(F1, truth)))
    assert apps * 20 <= apps1
    assert tc.relmax(F, truth) <= 2 * max(tc.relmax(F1, truth), 64 * tc.eps_of(np.float64))


# ---- declarations -----------------------------------------------------------------------------------------------------------------
def test_declared_exported_bound_and_built(eu):
    import ctypes
    import re
    from exponentialutilities_jl_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "expv_mi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    for name, nargs in (("expv_mi_op_norm_power", 8), ("expv_mi_host_normest_signs", 4), ("expv_mi_host_taylor_params_power", 6),
                        ("expv_mi_expv_taylor_power", 13)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
    assert "op_normest.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_normest.hip"))
    for name in ("expv_taylor_power", "expv_taylor_power_", "host_taylor_params_power", "host_normest_signs"):
        assert hasattr(eu, name), name
    assert hasattr(eu.MIOperator, "norm_power")
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert ":expv_mi_expv_taylor_power, lib" in src and ":expv_mi_op_norm_power, lib" in src
