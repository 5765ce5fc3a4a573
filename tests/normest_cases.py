"""The block 1-norm estimator of expv_mi_op_norm_power restated in numpy, the reference's whole Taylor parameter search by brute
force, and the operators their tests run on.

restated() is Algorithm 2.4 of Higham & Tisseur (2000) with t = 2, itmax = 5 in the control flow of scipy's _onenormest_core, with
every deterministic rule of include/expv_mi.h: the start block (1/n, +-1/n), signs from sign_hash() on natural rows, ties to the
smaller natural index, "all n signs agree" as the parallel test, fp64 column sums, and after every application the exact power of
two that brings the INPUT column's maximum (complex: max(|re|, |im|)) to [1, 2), the exponents summed in integers.  It runs in the
operator's element type or in a wider one (`arith`); a committed case has the same trace in both.

EXITS lists which exit of the loop every case takes, for p = 2, 5, 9 in the infinity norm (the CPU test asserts it)."""
import math

import numpy as np
import scipy.sparse as sp

from tests import expv_taylor_cases as tc

ITMAX, TOP, M_MAX, P_MAX = 5, 12, 55, 8
EXIT_NO_GROWTH, EXIT_ITMAX, EXIT_PARALLEL, EXIT_HMAX_IS_BEST, EXIT_VISITED, EXIT_NONFINITE, EXIT_EXACT = 1, 2, 3, 4, 5, 6, 7
_M1, _M2, _SALT = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53), np.uint64(0x9e3779b97f4a7c15)


def mix64(h):
    h = np.asarray(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint64(33))
        h = h * _M1
        h = h ^ (h >> np.uint64(33))
        h = h * _M2
        h = h ^ (h >> np.uint64(33))
    return h


def sign_hash(n, col, attempt):
    """+-1 (int8) for natural rows 0 .. n - 1: the low bit of mix64(((i + 1) g) ^ (col << 32 | attempt))"""
    with np.errstate(over="ignore"):
        w = (np.arange(1, n + 1, dtype=np.uint64) * _SALT) ^ np.uint64((int(col) << 32) | int(attempt))
    return np.where(mix64(w) & np.uint64(1), 1, -1).astype(np.int8)


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------
def wider(T):
    """the arithmetic a trace is re-run in: fp64 for the 32-bit types, longdouble for the 64-bit ones"""
    T = np.dtype(T)
    if T == np.float32:
        return np.dtype(np.float64)
    if T == np.complex64:
        return np.dtype(np.complex128)
    return np.dtype(np.clongdouble if T.kind == "c" else np.longdouble)


def lim_of(T):
    return 126 if np.dtype(T) in (np.dtype(np.float32), np.dtype(np.complex64)) else 1022


class Applier:
    """y = M x for a CSR or dense M held in the arithmetic W (scipy has no longdouble products: the rows are summed by reduceat)"""

    def __init__(self, M, W):
        self.W = np.dtype(W)
        if sp.issparse(M):
            M = sp.csr_matrix(M)
            M.sort_indices()
            self.indptr, self.indices, self.data = M.indptr, M.indices, M.data.astype(self.W)
            self.dense = None
        else:
            self.dense = np.asarray(M).astype(self.W)
        self.n = M.shape[0]

    def __call__(self, X):
        if self.dense is not None:
            return (self.dense @ X).astype(self.W)
        Y = np.zeros((self.n, X.shape[1]), dtype=self.W)
        rows = np.flatnonzero(np.diff(self.indptr) > 0)
        for k in range(X.shape[1]):
            prod = self.data * X[self.indices, k]
            if prod.size:
                Y[rows, k] = np.add.reduceat(prod, self.indptr[rows])
        return Y


def measure(x):
    x = np.asarray(x)
    if x.size == 0:
        return 0.0
    return max(np.max(np.abs(x.real)), np.max(np.abs(x.imag))) if x.dtype.kind == "c" else np.max(np.abs(x))


def exponent_of(m, lim):
    """floor(log2 m), clamped; 0 for a zero or non-finite maximum"""
    if not np.isfinite(m) or m <= 0 or m < np.finfo(np.float64).tiny:
        return 0
    return int(min(max(int(np.frexp(m)[1]) - 1, -lim), lim))


def power_apply(op, sigma, X, p, lim):
    """(M - sigma I)^p X with the device's scalings: (columns, their summed exponents)"""
    W = op.W
    E = [0] * X.shape[1]
    X = X.astype(W)
    s = W.type(sigma)
    for _ in range(p):
        e = [exponent_of(measure(X[:, k]), lim) for k in range(X.shape[1])]
        Y = (op(X) - s * X).astype(W)
        for k in range(X.shape[1]):
            Y[:, k] = np.ldexp(Y[:, k].real, -e[k]) + (1j * np.ldexp(Y[:, k].imag, -e[k]) if W.kind == "c" else 0)
            E[k] += e[k]
        X = Y.astype(W)
    return X, E


def _absw(Y, W):
    """|y| in the arithmetic the sums run in: fp64 (the device's), or W when that is wider"""
    wide = np.dtype(W).itemsize > (16 if np.dtype(W).kind == "c" else 8)
    return np.abs(Y) if wide else np.abs(Y.astype(np.complex128 if Y.dtype.kind == "c" else np.float64))


def restated(A, p, sigma=0.0, which=0, T=None, arith=None):
    """(est, trace) of ||(A - sigma I)^p||: which = 0 the infinity norm, 1 the 1-norm.  trace: iterations, exit, index, hist,
    resamples, applications, reads."""
    T = np.dtype(A.dtype if T is None else T)
    W = np.dtype(T if arith is None else arith)
    n = A.shape[0]
    lim = lim_of(T)
    is_c = T.kind == "c"
    AH = A.conj().T
    sig = complex(sigma) if is_c else float(np.real(sigma))
    if which == 1:
        fwd, bwd, s_f, s_b = Applier(A, W), Applier(AH, W), sig, np.conj(sig)
    else:
        fwd, bwd, s_f, s_b = Applier(AH, W), Applier(A, W), np.conj(sig), sig
    tr = {"iterations": 1, "exit": 0, "index": -1, "hist": [], "resamples": 0, "applications": 0, "reads": 0}

    def colsums(Y, E):
        a = _absw(Y, W)
        return [float(np.ldexp(a[:, k].sum(), E[k])) for k in range(Y.shape[1])]

    if n <= 2:
        X = np.eye(n, 2, dtype=W)
        Y, E = power_apply(fwd, s_f, X, p, lim)
        cs = colsums(Y, E)[:n] + [0.0] * (2 - n)
        tr.update(exit=EXIT_EXACT, index=1 if cs[1] > cs[0] else 0, applications=p, reads=1)
        return max(cs), tr

    attempt = 0
    while np.all(sign_hash(n, 1, attempt) > 0):
        attempt += 1
        tr["resamples"] += 1
    draws = attempt + 1
    inv_n = np.finfo(T).dtype.type(1.0 / n)
    X = np.empty((n, 2), dtype=W)
    X[:, 0] = inv_n
    X[:, 1] = sign_hash(n, 1, attempt) * W.type(inv_n)
    S = np.zeros((n, 2), dtype=W)
    est = est_old = 0.0
    ind, hist, ind_best, k = [], [], -1, 1
    with np.errstate(all="ignore"):
        while True:
            Y, E = power_apply(fwd, s_f, X, p, lim)
            tr["applications"] += p
            tr["reads"] += 1
            cs = colsums(Y, E)
            if not all(math.isfinite(c) or c == math.inf for c in cs) or any(c != c for c in cs):
                est, tr["exit"] = math.nan, EXIT_NONFINITE
                break
            best_j = 1 if cs[1] > cs[0] else 0
            est = cs[best_j]
            if (est > est_old or k == 2) and k >= 2:
                ind_best = ind[best_j]
            if k >= 2 and est <= est_old:
                est, tr["exit"] = est_old, EXIT_NO_GROWTH
                break
            est_old = est
            if k > ITMAX:
                tr["exit"] = EXIT_ITMAX
                break
            S_old = S
            if is_c:
                Yw = Y.astype(np.clongdouble if W.itemsize > 16 else np.complex128)
                a = np.abs(Yw)
                S = np.where(a == 0, 1.0, Yw / np.where(a == 0, 1.0, a)).astype(T).astype(W)
            else:
                S = np.where(Y < 0, -1.0, 1.0).astype(W)
                par = lambda v, M: any(np.count_nonzero(v == M[:, j]) == n for j in range(M.shape[1]))      # noqa: E731
                if all(par(S[:, q], S_old) for q in range(2)):
                    tr["exit"] = EXIT_PARALLEL
                    break
                for q in range(2):
                    while par(S[:, q], S_old) or (q == 1 and np.count_nonzero(S[:, 0] == S[:, 1]) == n):
                        S[:, q] = sign_hash(n, q, draws)
                        draws += 1
                        tr["resamples"] += 1
                        tr["reads"] += 1
            Z, Eb = power_apply(bwd, s_b, S, p, lim)
            tr["applications"] += p
            tr["reads"] += 1
            emax = max(Eb)
            a = _absw(Z, W)
            h = np.maximum(np.ldexp(a[:, 0], Eb[0] - emax), np.ldexp(a[:, 1], Eb[1] - emax))
            h = np.where(h != h, 0.0, h)
            order = np.lexsort((np.arange(n), -h))[:TOP]      # value descending, ties to the smaller index
            top = [int(i) for i in order]
            if k >= 2 and top[0] == ind_best:
                tr["exit"] = EXIT_HMAX_IS_BEST
                break
            want = min(len(top), 2 + len(hist))
            if top[0] in hist and top[1] in hist:
                tr["exit"] = EXIT_VISITED
                break
            ind = [i for i in top[:want] if i not in hist] + [i for i in top[:want] if i in hist]
            X = np.zeros((n, 2), dtype=W)
            X[ind[0], 0] = 1
            X[ind[1], 1] = 1
            hist += [i for i in ind[:2] if i not in hist]
            k += 1
    tr.update(iterations=k, index=ind_best, hist=list(hist))
    return est, tr


# ---- exact norms ---------------------------------------------------------------------------------------------------------------
_exact = {}


def shifted(A, sigma):
    """B = A - sigma I in 64-bit arithmetic, dense"""
    W = tc.wide(A.dtype)
    B = (A.toarray() if sp.issparse(A) else np.asarray(A)).astype(W)
    return B - W(sigma) * np.eye(A.shape[0], dtype=W)


def exact_norms(key, A, sigma, ps=(2, 5, 9)):
    """{p: (||B^p||_inf, ||B^p||_1, || |B|^p ||_inf, || |B|^p ||_1)} by dense powers, computed once per key"""
    if key not in _exact:
        out = {}
        for absolute in (False, True):
            B = shifted(A, sigma)
            if absolute:
                B = np.abs(B)
            pw = {1: B}
            pw[2] = B @ B
            pw[4] = pw[2] @ pw[2]
            pw[5] = pw[4] @ B
            pw[9] = pw[4] @ pw[5]
            for p in ps:
                M = np.abs(pw[p]) if p in pw else np.abs(np.linalg.matrix_power(B, p))
                out.setdefault(p, []).extend([float(M.sum(axis=1).max()), float(M.sum(axis=0).max())])
        _exact[key] = {p: tuple(v) for p, v in out.items()}
    return _exact[key]


def longest_row(A, sigma=1.0):
    if sp.issparse(A):
        return int(np.diff(sp.csr_matrix(A + sp.identity(A.shape[0], dtype=A.dtype, format="csr")).indptr).max())
    return A.shape[0]


# ---- the parameter search by brute force                                       ExponentialUtilitiesStaticArraysExt.jl:99-121 ----
def params_power(alpha1, d, theta):
    """(m*, s, p_used) of the reference's parameters(): d = (d_2 .. d_9)"""
    if alpha1 == 0:
        return 0, 1, 0
    if alpha1 <= 4 * theta[M_MAX - 1] * P_MAX * (P_MAX + 3) / (M_MAX * 1):
        m, s = tc.params(alpha1, theta)
        return m, s, 0
    best = None
    for p in range(2, P_MAX + 1):
        a = max(d[p - 2], d[p - 1])
        cand = min((m * math.ceil(a / theta[m - 1]), m) for m in range(p * (p - 1) - 1, M_MAX + 1))
        if best is None or cand < best[0]:
            best = (cand, p)
    (cost, m), p = best
    return m, max(cost // m, 1), p


# ---- operators -----------------------------------------------------------------------------------------------------------------
def block_triangular(m, T=np.float64):
    """[[L, C], [0, L]], L = tridiag(1, -2, 1) of order m, C = diag(1e3 (1 + u)) + superdiag(-500 (1 + u')): strongly non-normal"""
    r = np.random.default_rng(1)
    u, u1 = r.random(m), r.random(m - 1)
    L = sp.diags([np.ones(m - 1), -2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csr")
    Cc = sp.diags([1e3 * (1 + u), -500.0 * (1 + u1)], [0, 1], format="csr")
    A = sp.bmat([[L, Cc], [None, L]], format="csr")
    A.sort_indices()
    return A.astype(T).tocsr()


def schroedinger_coupled(m, T=np.complex128):
    """[[-i L, C], [0, -i L]] with a complex coupling C = diag(30 (1 + u) e^(i phi)) + superdiag(-12 (1 + u'))"""
    r = np.random.default_rng(5)
    u, u1, ph = r.random(m), r.random(m - 1), r.random(m)
    L = sp.diags([np.ones(m - 1), -2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csr") * (-1j)
    Cc = sp.diags([30.0 * (1 + u) * np.exp(2j * np.pi * ph), -12.0 * (1 + u1)], [0, 1], format="csr")
    A = sp.bmat([[L, Cc], [None, L]], format="csr")
    A.sort_indices()
    return A.astype(T).tocsr()


def hermitian(n, T=np.float64):
    """symmetric pentadiagonal with varying entries: its own adjoint"""
    r = np.random.default_rng(9)
    d0, d1, d2 = -2.0 - r.random(n), 0.5 + r.random(n - 1), 0.3 * r.random(n - 2)
    return sp.diags([d2, d1, d0, d1, d2], [-2, -1, 0, 1, 2], format="csr").astype(T).tocsr()


def row_scaled(A, seed, amp):
    """diag(1 + amp u^6) A: a few rows dominate, so that two columns find at least 0.9 of the norm of every tested power in both norms
    (a condition on the inputs, tests/test_normest_cpu.py; with flat random rows a t = 2 estimate reaches 0.55 .. 0.9 of it)"""
    d = 1.0 + amp * np.random.default_rng(100 + seed).random(A.shape[0]) ** 6
    if sp.issparse(A):
        return (sp.diags(d) @ A).astype(A.dtype).tocsr()
    return np.asfortranarray((d[:, None] * A).astype(A.dtype))


def circulant(n):
    """periodic stencil (0.5, 1, 2) with dyadic entries and n a power of two: every column sum of every power is the same and exact,
    so the second iteration cannot grow the estimate"""
    return sp.diags([np.full(n - 1, 0.5), np.full(n, 1.0), np.full(n - 1, 2.0), [2.0], [0.5]], [-1, 0, 1, -(n - 1), n - 1], format="csr")


def mean_diagonal(A):
    d = A.diagonal() if sp.issparse(A) else np.diag(A)
    return complex(d.sum() / A.shape[0]) if np.dtype(A.dtype).kind == "c" else float(d.sum() / A.shape[0])


_cases = {}
CASE_NAMES = ("bt200", "bt1537", "bt1537_f32", "random8_3001", "schroedinger_c128", "schroedinger_c64", "hermitian_777", "shuffled_band_2000", "dense300", "powerlaw_1000", "circulant_1024")


def case(name):
    """(A, sigma): the operator in its element type and the shift mu = tr(A) / n the Taylor entry would use"""
    if name not in _cases:
        A = {"bt200": lambda: block_triangular(200),
             "bt1537": lambda: block_triangular(1537),
             "bt1537_f32": lambda: block_triangular(1537, np.float32),
             "random8_3001": lambda: row_scaled(tc.random8(3001, np.float64), 3, 4.0),
             "schroedinger_c128": lambda: schroedinger_coupled(600),
             "schroedinger_c64": lambda: schroedinger_coupled(600, np.complex64),
             "hermitian_777": lambda: hermitian(777),
             "shuffled_band_2000": lambda: row_scaled(tc.shuffled_band(2000, np.float64)[0], 3, 4.0),
             "dense300": lambda: row_scaled(tc.dense(300, np.float32), 9, 20.0),
             "powerlaw_1000": lambda: row_scaled(tc.powerlaw(1000, np.float64), 10, 20.0),
             "circulant_1024": lambda: circulant(1024)}[name]()
        _cases[name] = (A, 0.0 if name == "circulant_1024" else mean_diagonal(A))
    return _cases[name]


# which exit each case takes, the same for p = 2, 5, 9 and both norms (asserted by tests/test_normest_cpu.py).  No input here
# reaches EXIT_ITMAX, EXIT_VISITED or EXIT_NONFINITE; EXIT_EXACT is n <= 2.
EXITS = {"bt200": EXIT_HMAX_IS_BEST, "bt1537": EXIT_HMAX_IS_BEST, "bt1537_f32": EXIT_HMAX_IS_BEST, "random8_3001": EXIT_HMAX_IS_BEST,
         "schroedinger_c128": EXIT_HMAX_IS_BEST, "schroedinger_c64": EXIT_HMAX_IS_BEST, "hermitian_777": EXIT_PARALLEL, "shuffled_band_2000": EXIT_HMAX_IS_BEST,
         "dense300": EXIT_HMAX_IS_BEST, "powerlaw_1000": EXIT_HMAX_IS_BEST, "circulant_1024": EXIT_NO_GROWTH}


# ---- the series behind given parameters ------------------------------------------------------------------------------------------
def restated_series(t, A, b, m, s, mu, tol, arith=None):
    """exp(tA)b by the truncated Taylor series of tests/expv_taylor_cases.py:restated with (m*, s) GIVEN, in the element type of A or in
    `arith`.  Returns (F, applications)."""
    T = np.dtype(A.dtype)
    W = np.dtype(T if arith is None else arith)
    R = np.finfo(W).dtype.type
    op = Applier(A, W)
    muW, tolR = W.type(mu), R(tol)
    eta = W.type(np.exp(np.clongdouble(mu) * np.clongdouble(t) / s)) if W.kind == "c" else W.type(np.exp(np.longdouble(np.real(mu)) * np.longdouble(np.real(t)) / s))
    F = np.array(b, dtype=W)
    v = F.copy()
    apps = 0
    with np.errstate(all="ignore"):
        for _ in range(s):
            c1 = np.max(np.abs(v))
            if c1 != 0:
                for j in range(1, m + 1):
                    c = W.type(complex(t) / s / j) if W.kind == "c" else W.type(float(np.real(t)) / s / j)
                    v = ((op(v[:, None])[:, 0] - muW * v) * c).astype(W)
                    F = (F + v).astype(W)
                    apps += 1
                    c2, nF = np.max(np.abs(v)), np.max(np.abs(F))
                    if R(c1 + c2) <= R(tolR * nF):
                        break
                    c1 = c2
            if eta != 1:
                F = (F * eta).astype(W)
            v = F.copy()
            if not np.all(np.isfinite(v)):
                break
    return F, apps


def restated_d(A, t, mu):
    """d_2 .. d_9 = |t| est_p^(1/p) from the restated estimator in the infinity norm"""
    return [abs(t) * restated(A, p, mu, 0)[0] ** (1.0 / p) for p in range(2, 10)]
