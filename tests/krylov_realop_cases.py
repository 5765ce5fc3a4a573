"""Inputs of the mixed-call tests (a real operator with complex vectors: tests/test_krylov_realop_cpu.py,
tests/test_gpu_krylov_realop.py).  Everything is seeded and small; a case is built once per process and shared."""
import functools

import numpy as np
import scipy.sparse as sp

REALS = (np.float64, np.float32)
TOL = 1e-12            # device vs oracle at the same m, 64-bit types: the TOL of tests/test_gpu_parity.py
TOL_TRUTH = 1e-10      # against scipy.linalg.expm(tA) b in the converged regime
TOL32 = 3e-5           # the 32-bit types, as tests/test_gpu_parity.py has it
MUL_N = (1, 127, 128, 129, 513, 2001)      # around a slice of the real type (128 rows fp64, 256 fp32), several workgroups
ARNOLDI_SHAPES = ((20, 5, 0), (513, 30, 0), (2001, 17, 3), (4099, 40, 0))      # windows of <= 8, 9..16 and > 16 columns: one, two and
                                                                               # more chunks of DotChunk<cplx>::CH = 8


def complex_of(R):
    return np.dtype(np.complex64 if np.dtype(R) == np.float32 else np.complex128)


def unit_roundoff(R):
    return 2.0 ** -24 if np.dtype(R) == np.float32 else 2.0 ** -53


def cvector(n, R=np.float64, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(complex_of(R))


@functools.lru_cache(maxsize=None)
def sell5(n, R=np.float64, seed=11, per_row=5, diag=-2.0):
    """`per_row` random entries per row (distinct columns anywhere) and a diagonal shift: regular rows, SELL slots, no diagonal form"""
    rng = np.random.default_rng(seed + n)
    k = min(per_row, n)
    cols = np.stack([rng.choice(n, size=k, replace=False) for _ in range(n)]) if n > k else np.tile(np.arange(n), (n, 1))
    rows = np.repeat(np.arange(n), k)
    vals = rng.standard_normal(n * k) / np.sqrt(k)
    A = sp.csr_matrix((vals, (rows, cols.ravel())), shape=(n, n))
    if diag:
        A = A + diag * sp.identity(n, format="csr")
    A.sum_duplicates()
    A.sort_indices()
    return A.astype(R).tocsr()


# The factorisation comparisons (H, V against the oracle at 1e-12) need an operator on which arnoldi! itself is well conditioned: on
# the random rows above two runs of the ORACLE that differ only in the summation order inside a row move H by 9e-8 at (n, m) =
# (513, 30), 8e-5 at (4099, 40) and O(1) at (300, 66) -- rounding-level perturbations grow with every step there, whoever computes.
# On the project's Toeplitz band (tests/_util.py: c2_operator) the same experiment moves H by 1e-15 at every shape used here, and a
# symmetric permutation of it has the same H in exact arithmetic while its columns lie anywhere: SELL slots with far gathers.
C2_OFFSETS = (-2, -1, 0, 1, 2)
C2_VALS = (0.3, 1.2, -2.0, 0.8, -0.1)


def band5(n, R=np.float64, offsets=C2_OFFSETS, vals=C2_VALS):
    return sp.diags([np.full(n - abs(o), v) for o, v in zip(offsets, vals)], offsets, shape=(n, n), format="csr").astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def scattered_band(n, R=np.float64, seed=5):
    """P c2 P' for a random permutation P: five entries per row in random columns, the Krylov recurrence of the band"""
    p = np.random.default_rng(seed + n).permutation(n)
    A = band5(n)[p][:, p].tocsr()
    A.sort_indices()
    return A.astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def scattered_sym(n, R=np.float64, seed=6):
    """P S P' of the symmetric band (sym5 below): regular rows in random columns, symmetric (lanczos! on SELL slots)"""
    p = np.random.default_rng(seed + n).permutation(n)
    A = band5(n, np.float64, C2_OFFSETS, (0.5, 1.0, -3.0, 1.0, 0.5))[p][:, p].tocsr()
    A.sort_indices()
    return A.astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def scattered_band_long_row(n=600, R=np.float64, seed=13, long_row=200):
    """the same with one row of `long_row` small entries: SELL slots up to a cut + overflow entries"""
    rng = np.random.default_rng(seed)
    A = scattered_band(n).tolil()
    A[n // 3, rng.choice(n, size=long_row, replace=False)] = rng.standard_normal(long_row) * 0.01
    A = A.tocsr()
    A.sort_indices()
    return A.astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def grid_band(n=1000, R=np.float64):
    """offsets {-37, -1, 0, 1, 37} with the band's values: the general diagonal form"""
    return band5(n, R, (-37, -1, 0, 1, 37))


@functools.lru_cache(maxsize=None)
def dense_band(n=67, R=np.float64):
    return np.asfortranarray(band5(n, R).toarray())


@functools.lru_cache(maxsize=None)
def gdia(n=1000, R=np.float64, seed=12, sym=False):
    """the general diagonal form: offsets {-37, -1, 0, 1, 37} with random values"""
    rng = np.random.default_rng(seed)
    offs = (-37, -1, 0, 1, 37)
    diags = {o: rng.standard_normal(n - abs(o)) * 0.5 for o in offs}
    if sym:
        for o in offs:
            if o > 0:
                diags[o] = diags[-o]
    diags[0] = diags[0] - 2.0
    return sp.diags([diags[o] for o in offs], offs, shape=(n, n), format="csr").astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def overflow(n=600, R=np.float64, seed=13, long_row=200):
    """rows with overflow entries: 5 random entries per row and one row of `long_row`"""
    rng = np.random.default_rng(seed)
    A = sell5(n, np.float64, seed).tolil()
    cols = rng.choice(n, size=long_row, replace=False)
    A[n // 3, cols] = rng.standard_normal(long_row) / np.sqrt(long_row)
    A = A.tocsr()
    A.sort_indices()
    return A.astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def dense(n=67, R=np.float64, seed=14):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.standard_normal((n, n)) / np.sqrt(n) - 1.5 * np.eye(n)).astype(R))


@functools.lru_cache(maxsize=None)
def permuted_band(n=2001, R=np.float64, seed=15):
    """a band of half-width 3 under a random symmetric permutation: creation reorders it (reorder_info)"""
    rng = np.random.default_rng(seed)
    offs = (-3, -2, -1, 0, 1, 2, 3)
    B = sp.diags([rng.standard_normal(n - abs(o)) * 0.4 - (2.0 if o == 0 else 0.0) for o in offs], offs, shape=(n, n), format="csr")
    p = rng.permutation(n)
    A = B[p][:, p].tocsr()
    A.sort_indices()
    return A.astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def sym5(n, R=np.float64):
    """the symmetric 5-diagonal operator (Lanczos)"""
    vals = (0.5, 1.0, -3.0, 1.0, 0.5)
    return sp.diags([np.full(n - abs(o), v) for o, v in zip((-2, -1, 0, 1, 2), vals)], (-2, -1, 0, 1, 2), shape=(n, n), format="csr").astype(R).tocsr()


@functools.lru_cache(maxsize=None)
def sym_sell(n, R=np.float64, seed=16):
    """a symmetric operator on SELL slots (no band): (S + S') / 2 of random rows"""
    S = sell5(n, np.float64, seed, diag=0.0)
    A = ((S + S.T) * 0.5 - 2.0 * sp.identity(n)).tocsr()
    A.sort_indices()
    return A.astype(R).tocsr()


def as_dense(A):
    return np.asarray(A.toarray() if sp.issparse(A) else A)


def mul_bound(A, x, R):
    """per real component: |y - A x| <= (k + 2) u (|A| |x|), k = stored entries of the row (n for dense), u the unit roundoff of R.
    Derived: an inner product of k terms accumulated with one rounding per fma has the error gamma_k (|a|' |x|) <= k u / (1 - k u);
    the two extra units cover 1 / (1 - k u) at these k and, on the path of two real applications, the final store.  |A| |x| is taken
    per component: |A| |Re x| for the real parts, |A| |Im x| for the imaginary ones."""
    u = unit_roundoff(R)
    if sp.issparse(A):
        absA = abs(A).astype(np.float64)
        k = np.diff(A.tocsr().indptr).astype(np.float64)
    else:
        absA = np.abs(np.asarray(A, dtype=np.float64))
        k = np.full(A.shape[0], float(A.shape[1]))
    x = np.asarray(x, dtype=np.complex128)
    return (k + 2.0) * u * (absA @ np.abs(x.real)), (k + 2.0) * u * (absA @ np.abs(x.imag))


def mul_reference(A, x):
    """A x in float64 / complex128 from the operator's stored values (exact to 2^-53 relative per term: far below either bound for
    Float32; for Float64 the reference's own error is of the size of the bound, so it is computed in extended precision)"""
    Ad = as_dense(A).astype(np.longdouble)
    x = np.asarray(x)
    re = Ad @ x.real.astype(np.longdouble)
    im = Ad @ x.imag.astype(np.longdouble)
    return re, im
