"""exp(tA)b for a REAL operator with a complex time and complex vectors (expv_mi_expv_taylor_realop): the cases its CPU and GPU tests
share.  The operators, the vectors, the numpy restatement (which already runs a real A in a complex element type), the norm and the
times come from tests/expv_taylor_cases.py; this file only names the combinations."""
import numpy as np

from tests import expv_taylor_cases as tc

REALS = [np.float64, np.float32]
# every slice and pack boundary of both operator types: 128 rows are one SELL slice of a Float64 operator, 256 of a Float32 one
SMALL_N = (1, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
BAR = 8.0      # tests/test_gpu_expv_taylor.py: the device differs from the restatement only in summation order inside a row and in contraction


def complex_of(R):
    return np.dtype(np.complex64 if np.dtype(R).itemsize == 4 else np.complex128)


def schroedinger_t(A, alpha):
    """t = -i tau with |t| opnorm(A - mu I, Inf) = alpha"""
    return -1j * abs(tc.t_for(A, alpha))


def ray_t(A, alpha):
    """t on the ray exp(0.3 i) with the same alpha"""
    return tc.t_for(A, alpha, True)


# (name, operator, alpha, t): the two cases of the slice-boundary test, Schroedinger on the Laplacian at alpha = 10 (s = 2: the
# 64-bit restatement stays below 64 eps; one stage would not) and a random sparse operator along the ray at alpha = 40
SMALL_CASES = [("laplacian", tc.laplacian, 10.0, schroedinger_t), ("random8", tc.random8, 40.0, ray_t)]
CASE_IDS = [c[0] for c in SMALL_CASES]


def cvector(n, R, seed=0):
    """a complex vector of the operator's precision"""
    return tc.vector(n, complex_of(R), seed)


def plan_and_restatement(A, b, t, theta_tables, precision=0, opnorm=None):
    """(mu, alpha, longest row, table, F, info) of the restatement in the operator's complex type"""
    R = np.dtype(A.dtype)
    Cd = complex_of(R)
    tab = tc.table_of(R, precision)
    mu, alpha, longest = tc.shift_norm(A, t)
    if opnorm is not None:
        mu, alpha = 0.0, abs(t) * opnorm
    F, info = tc.restated(t, A, b, Cd, alpha, theta_tables[tab], tc.TOL[tab], mu)
    return mu, alpha, longest, tab, F, info
