"""Inputs and CPU sides for phi!(out, A, k) of a dense device matrix (expv_mi_phi, csrc/dense_dev.hip); no device work here.

tests/test_gpu_phi_device.py runs these on the device, tests/test_phi_device_cpu.py checks the CPU sides against each other.

* restatement: the algorithm of expv_mi_phi in the ELEMENT TYPE with numpy products -- s = the smallest integer with |A|_1 2^-s <= 1,
  phi_k(A 2^-s) by its Taylor series to degree 18 / 10 (Paterson-Stockmeyer, tau = 4), phi_j = As phi_{j+1} + I / j! downwards, s
  recovery steps phi_0(2X) = phi_0(X)^2, phi_j(2X) = 2^-j (phi_0(X) phi_j(X) + sum_{i=1..j} phi_i(X) / (j - i)!).  What the same
  arithmetic gives on the CPU: the yardstick where the error grows with the scalings.
* truth: the first block row of scipy.linalg.expm of the block-augmented matrix [[A, I, 0, ..], [0, 0, I, ..], ..] in complex128.
  The truth at order K holds the truths of every k <= K, so one exponential per input serves all orders.
* closed forms that need no large exponential at any s: A = 0 (phi_j = I / j!), diagonal A (the scalar phi_j of every entry by the
  augmented trick on (k + 1) x (k + 1)), A = a E_12 (phi_j = I / j! + a / (j + 1)! E_12)."""
import functools
import math

import numpy as np
import scipy.linalg as sl

TYPES = ("float64", "complex128", "float32", "complex64")
THETA = 1.0
TAU = 4
PARITY_BAR = {"float64": 1e-11, "complex128": 1e-11, "float32": 1e-4, "complex64": 1e-4}
PARITY_SIZES = (1, 2, 7, 33, 65, 96, 129)
PARITY_ORDERS = (1, 2, 4)
PARITY_NORMS = (0.3, 5.0, 30.0)
PARITY_FAMILIES = ("randn", "skew")


def real_type(T):
    return np.dtype(np.float32 if np.dtype(T) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)


def degree(T):
    """Taylor degree M: the smallest with 1 / (M + 1)! (1 - 1 / (M + 2))^-1 below the unit roundoff of the real type (k = 0 is the
    worst order)"""
    u = float(np.finfo(real_type(T)).eps) / 2
    M = 0
    while 1.0 / math.factorial(M + 1) / (1.0 - THETA / (M + 2)) > u:
        M += 1
    return M


def scalings(nA):
    """the smallest s >= 0 with nA 2^-s <= theta = 1, from the exponent of nA"""
    if not nA > THETA:
        return 0
    f, e = math.frexp(nA)
    return e - 1 if f == 0.5 else e


def norm1_f64(A):
    return float(np.linalg.norm(np.asarray(A).astype(np.complex128), 1))


def rel_err(E, ref):
    return float(np.linalg.norm(np.asarray(E).astype(np.complex128) - ref) / np.linalg.norm(ref))


def products(T, k, s):
    """matrix products one call launches: tau - 1 powers, M // tau Horner steps, k recurrence steps, one wide product per recovery"""
    return (TAU - 1) + degree(T) // TAU + k + s


# ------------------------------------------------------------------------------------------- the algorithm in the element type
def restatement(A, k, drop_recovery=0):
    """[phi_0(A), ..., phi_k(A)] by the algorithm of expv_mi_phi, every operation in A's own type.  Returns (list, M, s)."""
    A = np.asarray(A)
    T = A.dtype
    R = real_type(T).type
    n = A.shape[0]
    M, s = degree(T), scalings(norm1_f64(A))
    As = A * R(math.ldexp(1.0, -s))
    I = np.eye(n, dtype=T)
    c = [R(1.0 / math.factorial(i + k)) for i in range(M + 1)]
    P = [I, As, As @ As]
    P.append(P[2] @ As)
    P4 = P[2] @ P[2]
    acc = None
    for b in range(M // TAU, -1, -1):
        B = sum(c[b * TAU + l] * P[l] for l in range(min(TAU, M + 1 - b * TAU)))
        acc = B if acc is None else acc @ P4 + B
    phis = [None] * (k + 1)
    phis[k] = acc
    for j in range(k - 1, -1, -1):
        phis[j] = As @ phis[j + 1] + R(1.0 / math.factorial(j)) * I
    for _ in range(s - drop_recovery):
        old = phis
        phis = [old[0] @ old[0]]
        for j in range(1, k + 1):
            acc = old[0] @ old[j]
            for i in range(1, j + 1):
                acc = acc + R(1.0 / math.factorial(j - i)) * old[i]
            phis.append(R(math.ldexp(1.0, -j)) * acc)
    assert all(p.dtype == T for p in phis)
    return phis, M, s


# ------------------------------------------------------------------------------------------- truths
def augmented(A, k):
    """W with exp(W)[:n, j n:(j + 1) n] = phi_j(A)"""
    A = np.asarray(A).astype(np.complex128)
    n = A.shape[0]
    W = np.zeros(((k + 1) * n, (k + 1) * n), dtype=np.complex128)
    W[:n, :n] = A
    for j in range(k):
        W[j * n:(j + 1) * n, (j + 1) * n:(j + 2) * n] = np.eye(n)
    return W


def truth(A, k):
    """[phi_0(A), ..., phi_k(A)] in complex128 of the matrix as stored"""
    n = np.asarray(A).shape[0]
    E = sl.expm(augmented(A, k))
    return [E[:n, j * n:(j + 1) * n] for j in range(k + 1)]


def zero_truth(T, n, k):
    """A = 0: phi_j = I / j!, exactly what the element type holds of 1 / j!"""
    R = real_type(T).type
    return [np.asarray(R(1.0 / math.factorial(j)) * np.eye(n), dtype=T) for j in range(k + 1)]


def diagonal_truth(d, k):
    """phi_j(diag(d)): the scalar phi_j of every entry, by the augmented trick on (k + 1) x (k + 1)"""
    d = np.asarray(d).astype(np.complex128)
    vals = np.array([sl.expm(augmented(np.array([[z]]), k))[0, :] for z in d])
    return [np.diag(vals[:, j]) for j in range(k + 1)]


def nilpotent(T, n, a):
    A = np.zeros((n, n), dtype=T, order="F")
    A[0, 1] = a
    return A


def nilpotent_truth(A, k):
    """A = a E_12, A^2 = 0: phi_j = I / j! + a / (j + 1)! E_12"""
    n = A.shape[0]
    out = []
    for j in range(k + 1):
        P = np.eye(n, dtype=np.complex128) / math.factorial(j)
        P[0, 1] += complex(A[0, 1]) / math.factorial(j + 1)
        out.append(P)
    return out


# ------------------------------------------------------------------------------------------- inputs
def matrix(tname, n, norm1, family, seed=None):
    """An n x n matrix of the family scaled to the 1-norm `norm1`, in the element type, column-major and read-only.  randn: as drawn;
    skew: G - G^H (exp is unitary); negsemi: -G G^H (Hermitian, no positive eigenvalue)."""
    T = np.dtype(tname)
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    G = rng.standard_normal((n, n))
    if T.kind == "c":
        G = G + 1j * rng.standard_normal((n, n))
    if family == "skew":
        G = G - G.conj().T
        if n == 1 and T.kind != "c":
            G = G + 1.0           # (a real skew 1 x 1 matrix is zero: keep a norm to scale)
    elif family == "negsemi":
        G = -(G @ G.conj().T)
    elif family != "randn":
        raise ValueError(family)
    A = np.asfortranarray((G * (norm1 / np.linalg.norm(G, 1))).astype(T))
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def case(tname, n, norm1, family, kmax=max(PARITY_ORDERS)):
    """(A, truths up to kmax): one exponential per input, shared by every test that needs it"""
    A = matrix(tname, n, norm1, family)
    ref = truth(A, kmax)
    for r in ref:
        r.setflags(write=False)
    return A, ref


def column_heavy(tname, n, norm1):
    """one column carries the 1-norm over n equal entries: the infinity norm is n times smaller"""
    A = np.zeros((n, n), dtype=tname, order="F")
    A[:, 0] = norm1 / n
    return A
