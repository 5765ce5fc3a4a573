"""The basis-free phiv_timestep (expv_mi_phiv_taylor) restated in numpy:  w = sum_{k=0..p} t^k phi_k(tA) u_k,  B = [u_0 ... u_p].

Al-Mohy & Higham (SIAM J. Sci. Comput. 33, 2011), Theorem 2.1: with W = [u_p, ..., u_1] and J the p x p upward shift, the first n rows of
exp(t [A W; 0 J]) [u_0; e_p] are that sum.  restated() runs the truncated Taylor series of tests/expv_taylor_cases.py on the augmented
matrix WITHOUT forming it: the p tail components of every term are data-independent and computed in (complex) double, the n head
components in the element type T, and the stopping test has the floor tail_j = |zeta_j|_inf U so that a call whose u_0 is zero does not
stop before the forcing has entered."""
import math

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

from tests import expv_taylor_cases as tc

PMAX = 8


def abs64(x):
    """|x| of every element in 64-bit arithmetic, CORRECTLY ROUNDED for the complex types, as the device's plan takes it (hypot is
    good to an ulp, and which ulp differs between math libraries): numpy's hypot, then every element re-rounded from 200 bits"""
    x = np.asarray(x)
    if x.dtype.kind != "c":
        return np.abs(x.astype(np.float64))
    import mpmath as mp
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    out = np.hypot(re, im)
    with mp.workprec(200):
        for i in np.ndindex(out.shape):
            out[i] = float(mp.sqrt(mp.mpf(float(re[i])) ** 2 + mp.mpf(float(im[i])) ** 2))
    return out


def nu_of(wmax):
    """2^(-ceil(log2 wmax)), 1 for wmax = 0"""
    if wmax == 0:
        return 1.0
    f, e = math.frexp(wmax)      # wmax = f 2^e, 0.5 <= f < 1
    return math.ldexp(1.0, -(e - 1 if f == 0.5 else e))


def plan(t, A, B, opnorm=None):
    """(mu, alpha, nu, U, longest row) in 64-bit arithmetic.  opnorm: a matrix-free operator (mu = 0, the caller's bound for the rows of A)"""
    n, p = B.shape[0], B.shape[1] - 1
    Wd = tc.wide(B.dtype)
    ab = abs64(B[:, 1:]) if p else np.zeros((n, 0))
    U = float(ab.max()) if ab.size else 0.0
    rows_b = np.zeros(n)
    for k in range(p):
        rows_b = rows_b + ab[:, k]
    nu = nu_of(float(rows_b.max()) if n else 0.0)
    if opnorm is not None:
        mu, rows, longest = 0.0, np.full(n, float(opnorm)), 0
    elif sp.issparse(A):
        A = sp.csr_matrix(A).astype(Wd)
        mu = A.diagonal().sum() / (n + p)
        rows = np.asarray(abs((A - mu * sp.identity(n, dtype=Wd, format="csr")).tocsr()).sum(axis=1)).ravel()
        longest = int(np.diff(A.indptr).max()) + 1 if n else 0
    else:
        A = np.asarray(A, dtype=Wd)
        mu = np.trace(A) / (n + p)
        rows = np.abs(A - mu * np.eye(n)).sum(axis=1)
        longest = n
    top = float((rows + nu * rows_b).max()) if n else 0.0
    if p > 0:
        top = max(top, 1.0 + abs(mu))
    return mu, abs(t) * top, nu, U, longest


def restated(t, A, B, T, theta, tol, opnorm=None):
    """sum t^k phi_k(tA) u_k in element type T.  Returns (F, info): m, s, applications, early_stages, alpha, mu, nu, U, longest,
    and skipped = the term launches (of s m) whose coefficients g_j, rounded to T, are all zero."""
    T = np.dtype(T)
    R = np.finfo(T).dtype.type
    cx = T.kind == "c"
    n, p = B.shape[0], B.shape[1] - 1
    B = np.asarray(B, dtype=T)
    mu, alpha, nu, U, longest = plan(t, A, B, opnorm)
    A = sp.csr_matrix(A).astype(T) if sp.issparse(A) else np.asarray(A, dtype=T)
    m, s = tc.params(alpha, theta)
    z = (lambda x: complex(x)) if cx else (lambda x: float(np.real(x)))
    h = z(t) / s
    muT, tolR = T.type(mu), R(tol)
    eta = T.type(np.exp(complex(mu) * complex(t) / s)) if cx else T.type(math.exp(float(np.real(mu)) * float(np.real(t)) / s))
    F = B[:, 0].copy()
    v = F.copy()
    info = {"m": m, "s": s, "applications": 0, "early_stages": 0, "alpha": alpha, "mu": mu, "nu": nu, "U": U, "longest": longest, "skipped": 0}
    norm = lambda zeta: max((abs(x) for x in zeta), default=0.0)
    with np.errstate(all="ignore"):
        for stage in range(s):
            tau = stage * h
            zeta = [z(1.0)] * p      # zeta[i - 1] = tau^(p - i) / (p - i)!,  i = 1 .. p
            for i in range(p - 1, 0, -1):
                zeta[i - 1] = zeta[i] * tau / (p - i)
            c1 = max(float(np.max(np.abs(v))) if n else 0.0, norm(zeta) * U)
            stopped = c1 == 0
            if stopped:
                info["early_stages"] += 1
            for j in range(1, m + 1):
                g = [(h / j) * x for x in zeta]
                zeta = [(h / j) * ((zeta[i + 1] if i + 1 < p else 0.0) - z(mu) * zeta[i]) for i in range(p)]
                gT = [T.type(x) for x in g]
                if not any(x != 0 for x in gT):
                    info["skipped"] += 1
                if stopped:
                    continue
                c = T.type(h / j)
                v = ((A @ v - muT * v) * c).astype(T)
                for k in range(1, p + 1):
                    if gT[p - k] != 0:
                        v = (v + gT[p - k] * B[:, k]).astype(T)
                F = (F + v).astype(T)
                info["applications"] += 1
                c2 = max(float(np.max(np.abs(v))), norm(zeta) * U)
                if R(c1 + c2) <= R(tolR * np.max(np.abs(F))):
                    info["early_stages"] += int(j < m)
                    stopped = True
                c1 = c2
            if eta != 1:
                F = (F * eta).astype(T)
            v = F.copy()
    return F, info


def augmented(A, B):
    """[A W; 0 J] in the wide type and the starting vector [u_0; e_p]"""
    n, p = B.shape[0], B.shape[1] - 1
    Wd = tc.wide(B.dtype)
    M = np.zeros((n + p, n + p), dtype=Wd)
    M[:n, :n] = (A.toarray() if sp.issparse(A) else np.asarray(A)).astype(Wd)
    for i in range(1, p + 1):
        M[:n, n + i - 1] = B[:, p + 1 - i]
        if i > 1:
            M[n + i - 2, n + i - 1] = 1.0
    x = np.zeros(n + p, dtype=Wd)
    x[:n] = B[:, 0]
    if p:
        x[n + p - 1] = 1.0
    return M, x


def truth(t, A, B):
    """the first n rows of scipy.linalg.expm(t [A W; 0 J]) [u_0; e_p] in the wide type"""
    M, x = augmented(A, B)
    return (sl.expm(t * M) @ x)[:B.shape[0]]


def block(n, p, T, seed=0, only_last=False):
    """B = [u_0 ... u_p]: standard normal entries, u_1 .. u_p divided by n; only_last: u_0 .. u_{p-1} = 0.
    The columns of W are columns of the augmented matrix, and its 1-norm sets the number of squarings in scipy's expm: with columns
    of 1-norm ~ n the truth itself is 60 .. 150 eps off (measured against the series in 80-bit arithmetic, which the restatement
    matches to 4 eps); with columns of 1-norm ~ 1 it is as good as for exp(tA)b."""
    r = tc.rng_of(n, 89, p, seed)
    B = r.standard_normal((n, p + 1))
    if np.dtype(T).kind == "c":
        B = B + 1j * r.standard_normal((n, p + 1))
    B[:, 1:] /= n
    if only_last:
        B[:, :p] = 0
    return np.asfortranarray(B.astype(T))


def t_for(A, B, alpha, complex_t=False):
    """the t (on the ray exp(0.3 i) when complex_t) with |t| opnorm(A - mu I, Inf) = alpha, mu = tr(A) / (n + p)"""
    n, p = B.shape[0], B.shape[1] - 1
    Wd = tc.wide(A.dtype)
    if sp.issparse(A):
        Aw = sp.csr_matrix(A).astype(Wd)
        mu = Aw.diagonal().sum() / (n + p)
        base = float(abs((Aw - mu * sp.identity(n, dtype=Wd, format="csr")).tocsr()).sum(axis=1).max())
    else:
        Aw = np.asarray(A, dtype=Wd)
        mu = np.trace(Aw) / (n + p)
        base = float(np.abs(Aw - mu * np.eye(n)).sum(axis=1).max())
    t = alpha / base if base > 0 else 1.0
    return t * complex(math.cos(0.3), math.sin(0.3)) if complex_t else t


# ---- the cases of tests/test_gpu_phiv_taylor.py (and of the restatement's own check in tests/test_phiv_taylor_cpu.py) ----------
SMALL_N = (1, 5, 63, 64, 65, 127, 128, 129, 257)
PS = (1, 2, 3, 8)
OPERATORS = ("tridiagonal", "random8", "dense")      # diagonal-form fused, SELL fused, mul! + update


def operator(kind, n, T):
    """The operators of tests/expv_taylor_cases.py, except for the scalars (n = 1) of random8 and dense, which are taken with
    |a| ~ 4 instead of |a| ~ 0.7, negative for the 64-bit types and positive for the 32-bit types:
      - |a - mu| = |a| p / (1 + p), so |t| |a - mu| = 40 makes t = 60 .. 90 for |a| ~ 0.7, and t J is a Jordan block of that size:
        scipy's expm of the 9 x 9 augmented matrix is 5e2 .. 1e5 eps off there (measured against the series in 80-bit arithmetic, which
        the restatement matches to 13 eps).  With a ~ +4 and a real type it is still 2e2 eps off (the result is e^60 large); with
        a ~ -4 it is within 10 eps.
      - with a < 0 the head row is one number in which c (a - mu) v and the forcing cancel.  At the alpha / s ~ 12 of the 2^-24 table
        what is left of a late term in single precision is rounding noise above tol |F|, and the term at which a stage stops moves by
        up to 7 when a changes by ONE ULP (the restatement against itself; s = 4), which the comparison of application counts cannot
        tell from a fault.  With a > 0 every term has the same sign and the count does not move; nor does it in double with a < 0
        (alpha / s ~ 9)."""
    if kind == "tridiagonal":
        return tc.laplacian(n, T)
    wide_type = np.dtype(T).itemsize >= (16 if np.dtype(T).kind == "c" else 8)
    if kind == "random8":
        return tc.random8(n, T, shift=(-3.0 if wide_type else 5.0) if n == 1 else 0.0)
    A = tc.dense(n, T)
    return np.asfortranarray(((-6.0 if wide_type else 6.0) * np.abs(A)).astype(T)) if n == 1 else A


def alpha_for(kind, T):
    """|t| opnorm(A - mu I, Inf): 40, and 10 for the -i Laplacian (tests/test_gpu_expv_taylor.py: the hump of the Schroedinger case)"""
    return 10.0 if (kind == "tridiagonal" and np.dtype(T).kind == "c") else 40.0


def parity_cases(T):
    """(n, p, only_last, complex_t) of the parity test and of the only-u_p test"""
    cts = (False, True) if np.dtype(T).kind == "c" else (False,)
    out = [(n, p, False, ct) for n in SMALL_N for p in PS for ct in cts]
    out += [(n, p, True, False) for n in (65, 257) for p in (2, 8)]
    return out
