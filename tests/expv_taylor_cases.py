"""The truncated-Taylor exp(tA)b (expv_mi_expv_taylor) restated in numpy, and the operators its tests run on.

restated() is the algorithm of ext/ExponentialUtilitiesStaticArraysExt.jl:124-163 of the reference with the library's documented
choices: the norm (alpha) and the theta table are arguments, it runs in any of the four element types, a zero v applies nothing,
and the stage factor exp(mu t / s) is skipped when it is exactly 1."""
import math

import numpy as np
import scipy.sparse as sp

M_MAX = 55
TOL = {0: 2.0 ** -53, 1: 2.0 ** -24}
DTYPES = [np.float64, np.complex128, np.float32, np.complex64]


def wide(T):
    return np.complex128 if np.dtype(T).kind == "c" else np.float64


def eps_of(T):
    return float(np.finfo(np.dtype(T)).eps)


def table_of(T, precision=0):
    """which table (0: 2^-53, 1: 2^-24) a call with `precision` on an operator of type T uses"""
    return 1 if (precision == 1 or np.dtype(T).itemsize <= (8 if np.dtype(T).kind == "c" else 4)) else 0


def theta_mp(m, bits, digits=60):
    """theta_m re-derived with mpmath (Al-Mohy & Higham 2011, section 3): the positive root of (-1)^m log(e^x T_m(-x)) = tol x below
    the first real zero of T_m(-x); theta_1 = 2 tol"""
    import mpmath as mp
    mp.mp.dps = digits
    tol = mp.mpf(2) ** -bits
    if m == 1:
        return float(2 * tol)

    def above(x):
        term, T = mp.mpf(1), mp.mpf(1)
        for k in range(1, m + 1):
            term = -term * x / k
            T += term
        return T <= 0 or (-1) ** m * (x + mp.log(T)) > tol * x

    lo, hi = mp.mpf(0), mp.mpf(2) ** -60
    while not above(hi):
        lo, hi = hi, 2 * hi
    for _ in range(210):
        mid = (lo + hi) / 2
        lo, hi = (lo, mid) if above(mid) else (mid, hi)
    return float((lo + hi) / 2)


def params(alpha, theta):
    """(m*, s): argmin over m of m ceil(alpha / theta_m), the first minimum on ties; alpha = 0 gives (0, 1)"""
    if alpha == 0:
        return 0, 1
    best = None
    for m in range(1, M_MAX + 1):
        s = math.ceil(alpha / theta[m - 1])
        if best is None or m * s < best[0]:
            best = (m * s, m, s)
    return best[1], best[2]


def shift_norm(A, t):
    """mu = tr(A) / n and alpha = |t| opnorm(A - mu I, Inf) in 64-bit arithmetic, + the longest row"""
    n = A.shape[0]
    W = wide(A.dtype)
    if sp.issparse(A):
        A = sp.csr_matrix(A).astype(W)
        mu = A.diagonal().sum() / n
        S = (A - mu * sp.identity(n, dtype=W, format="csr")).tocsr()
        rows = np.asarray(abs(S).sum(axis=1)).ravel()
        longest = int(np.diff(A.indptr).max()) + 1 if n else 0
    else:
        A = np.asarray(A, dtype=W)
        mu = np.trace(A) / n
        rows = np.abs(A - mu * np.eye(n)).sum(axis=1)
        longest = n
    return mu, abs(t) * float(rows.max()), longest


def restated(t, A, b, T, alpha, theta, tol, mu=None):
    """exp(tA)b in element type T.  Returns (F, info) with info = {m, s, applications, early_stages, nonfinite_stage}."""
    T = np.dtype(T)
    R = np.finfo(T).dtype.type
    n = A.shape[0]
    A = sp.csr_matrix(A).astype(T) if sp.issparse(A) else np.asarray(A, dtype=T)
    if mu is None:
        mu = shift_norm(A, t)[0]
    m, s = params(alpha, theta)
    muT, tolR = T.type(mu), R(tol)
    eta = T.type(np.exp(complex(mu) * complex(t) / s)) if T.kind == "c" else T.type(math.exp(float(np.real(mu)) * float(np.real(t)) / s))
    F = np.array(b, dtype=T)
    v = F.copy()
    info = {"m": m, "s": s, "applications": 0, "early_stages": 0, "nonfinite_stage": 0}
    with np.errstate(all="ignore"):
        for stage in range(s):
            c1 = np.max(np.abs(v)) if n else R(0)
            if c1 == 0:
                info["early_stages"] += 1      # a zero vector stays zero: nothing is applied
            else:
                for j in range(1, m + 1):
                    c = T.type(complex(t) / s / j) if T.kind == "c" else T.type(float(np.real(t)) / s / j)
                    v = ((A @ v - muT * v) * c).astype(T)
                    F = (F + v).astype(T)
                    info["applications"] += 1
                    c2, nF = np.max(np.abs(v)), np.max(np.abs(F))
                    if R(c1 + c2) <= R(tolR * nF):
                        info["early_stages"] += int(j < m)
                        break
                    c1 = c2
            if eta != 1:
                F = (F * eta).astype(T)
            v = F.copy()
            if not np.all(np.isfinite(v)):
                info["nonfinite_stage"] = stage + 1
                break
    return F, info


def relmax(a, b):
    """relative error in the max norm"""
    a, b = np.asarray(a), np.asarray(b)
    d = float(np.max(np.abs(b))) if b.size else 0.0
    return float(np.max(np.abs(a - b))) / (d if d > 0 else 1.0) if b.size else 0.0


# ---- operators ---------------------------------------------------------------------------------------------------------------
def rng_of(*key):
    return np.random.default_rng([20260 + k for k in key])


def laplacian(n, T):
    """tridiagonal (1, -2, 1), times -i for the complex types (the Schroedinger case): general diagonal form"""
    A = sp.diags([np.ones(max(n - 1, 0)), -2.0 * np.ones(n), np.ones(max(n - 1, 0))], [-1, 0, 1], shape=(n, n), format="csr")
    return (A * (-1j if np.dtype(T).kind == "c" else 1.0)).astype(T).tocsr()


def penta(n, T):
    """five non-symmetric diagonals with varying entries"""
    r = rng_of(n, 5)
    coef = {-2: 0.3, -1: 1.2, 0: -2.0, 1: 0.8, 2: -0.1}
    offs = [o for o in coef if abs(o) < n]
    d = [(0.5 + r.random(n - abs(o))) * coef[o] for o in offs]
    A = sp.diags(d, offs, shape=(n, n), format="csr")
    if np.dtype(T).kind == "c":
        A = A * (0.6 + 0.8j)
    return A.astype(T).tocsr()


def random8(n, T, shift=0.0):
    """8 entries per row at random columns (+ the diagonal): SELL slots, no diagonal form"""
    r = rng_of(n, 8)
    k = min(8, n)
    cols = np.stack([r.choice(n, size=k, replace=False) for _ in range(n)])
    vals = r.standard_normal((n, k)) / math.sqrt(k)
    if np.dtype(T).kind == "c":
        vals = vals + 1j * r.standard_normal((n, k)) / math.sqrt(k)
    A = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    A = A + sp.identity(n, format="csr") * (shift - 1.0)
    A.sum_duplicates()
    A.sort_indices()
    return A.astype(T).tocsr()


def powerlaw(n, T):
    """row lengths 1 .. n / 2 by a power law: the long rows overflow the SELL slots"""
    r = rng_of(n, 13)
    lens = np.minimum(n // 2, np.maximum(1, (3.0 * (1.0 - r.random(n)) ** -1.1).astype(np.int64)))
    lens[:: max(n // 7, 1)] = n // 2
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([r.choice(n, size=int(l), replace=False) for l in lens])
    vals = r.standard_normal(len(rows)) / np.sqrt(np.repeat(lens, lens))
    if np.dtype(T).kind == "c":
        vals = vals * np.exp(2j * np.pi * r.random(len(rows)))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n)) - sp.identity(n, format="csr")
    A.sum_duplicates()
    A.sort_indices()
    return A.astype(T).tocsr()


def dense(n, T):
    r = rng_of(n, 21)
    A = r.standard_normal((n, n)) / math.sqrt(n)
    if np.dtype(T).kind == "c":
        A = A + 1j * r.standard_normal((n, n)) / math.sqrt(n)
    return np.asfortranarray((A - 0.5 * np.eye(n)).astype(T))


def shuffled_band(n, T):
    """a band of half-width 3 in a random numbering: the creation reorders it.  Returns (A, the shuffle)"""
    r = rng_of(n, 34)
    offs = (-3, -1, 0, 1, 3)
    B = sp.diags([(0.5 + r.random(n - abs(o))) * c for o, c in zip(offs, (0.4, 1.0, -2.5, 0.9, 0.2))], offs, shape=(n, n), format="csr")
    if np.dtype(T).kind == "c":
        B = B * (0.8 - 0.6j)
    q = r.permutation(n)
    return B[q][:, q].astype(T).tocsr(), q


def vector(n, T, seed=0):
    r = rng_of(n, 55, seed)
    b = r.standard_normal(n)
    if np.dtype(T).kind == "c":
        b = b + 1j * r.standard_normal(n)
    return b.astype(T)


def t_for(A, alpha, complex_t=False):
    """the t (on the ray exp(0.3 i) when complex_t) that gives alpha = |t| opnorm(A - mu I, Inf)"""
    base = shift_norm(A, 1.0)[1]
    t = alpha / base if base > 0 else 1.0
    return t * complex(math.cos(0.3), math.sin(0.3)) if complex_t else t
