"""Inputs with a known answer for the dense device exponential (csrc/dense_dev.hip), and the CPU side of their checks; no device work here.

tests/test_gpu_expm_device_stress.py runs these on the device, tests/test_expm_device_cpu.py checks without one that the inputs have
the properties the device tests rely on (they pivot with fill, their pivots are decided far above rounding, a column sums to the
other side of a threshold in float32, ...).

* scattered_skew: skew-Hermitian k x k blocks scattered over a random permutation of the rows.  exp(A) is the same scatter of the
  k x k exponentials (block_reference: scipy on each block, milliseconds at any n), it is unitary, so no norm over- or underflows,
  every column's 1-norm is at most `norm1` whatever n is, and V - U ~ c exp(-A / 2) rotates inside every block: partial pivoting
  has to exchange rows there, with fill, and the scatter spreads a block's rows over many panels of the blocked LU.
* restatement: Higham 2005 without balancing in the ELEMENT TYPE (numpy matmul, LAPACK getrf / getrs of that type, coefficients cast
  to its real type) -- what the same arithmetic gives on the CPU, the yardstick where the error grows with the squarings.
* tied_hubs: 3 x 3 skew blocks with two EQUAL rows, scattered: every block's first pivot column holds the same largest value
  twice, bit for bit, and which of the two rows is taken decides whether the block exchanges rows once or twice.
* exchange_stats / pivot_gap: what LAPACK's partial pivoting does on a CPU-formed V - U, and by how much each pivot beats its
  runner-up (a plain elimination in double precision that skips the rows and columns a step leaves unchanged)."""
import functools
import math

import numpy as np
import scipy.linalg as sl

from oracle import krylov_oracle as ko

PADE = {3: ko._PADE_C3, 5: ko._PADE_C5, 7: ko._PADE_C7, 9: ko._PADE_C9, 13: ko._PADE_C13}
ORDER_THRESHOLDS = (0.015, 0.25, 0.95, 2.1)      # at the threshold: the lower order
THETA13 = 5.4
LU_NB, PANEL_THREADS = 32, 512                   # csrc/dense_dev.hip: panel width, threads of the panel kernel


def real_type(T):
    return np.dtype(np.float32 if np.dtype(T) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)


def expected_method(nA):
    """Pade order and squarings the thresholds give (exp_baseexp.jl / host_dense.h / dense_dev.hip)"""
    if nA <= 2.1:
        return (9 if nA > 0.95 else 7 if nA > 0.25 else 5 if nA > 0.015 else 3), 0
    return 13, max(0, math.ceil(math.log2(nA / THETA13)))


def norm1_f64(A):
    """opnorm(A, 1) with double-precision magnitudes and sums of the matrix as stored"""
    return float(np.linalg.norm(np.asarray(A).astype(np.complex128), 1))


# ------------------------------------------------------------------------------------------- scattered skew blocks
def scattered_skew(T, n, k, norm1, seed):
    """(A in the element type, column-major and read-only; the index sets of its blocks)"""
    T = np.dtype(T)
    rng = np.random.default_rng(seed)
    p = rng.permutation(n)
    A = np.zeros((n, n), dtype=np.complex128 if T.kind == "c" else np.float64)
    blocks = []
    for lo in range(0, n, k):
        idx = p[lo:lo + k]
        kk = len(idx)
        B = rng.standard_normal((kk, kk))
        if T.kind == "c":
            B = B + 1j * rng.standard_normal((kk, kk))
        K = B - B.conj().T
        nk = np.linalg.norm(K, 1)
        if nk > 0:                               # (a 1 x 1 real block stays 0)
            K = K * (norm1 / nk)
        A[np.ix_(idx, idx)] = K
        blocks.append(idx)
    A = np.asfortranarray(A.astype(T))
    A.setflags(write=False)
    return A, blocks


def block_reference(A, blocks):
    """exp(A) in complex128: scipy.linalg.expm of every (rounded) block, scattered back"""
    ref = np.zeros(A.shape, dtype=np.complex128)
    for idx in blocks:
        ref[np.ix_(idx, idx)] = sl.expm(A[np.ix_(idx, idx)].astype(np.complex128))
    return ref


def rel_err(E, ref):
    return float(np.linalg.norm(np.asarray(E).astype(np.complex128) - ref) / np.linalg.norm(ref))


# ------------------------------------------------------------------------------------------- the algorithm in the element type
def restatement(A):
    """Higham 2005 without balancing, every operation in A's own type.  Returns (exp(A), V - U, order, squarings)."""
    A = np.asarray(A)
    T, R = A.dtype, real_type(A.dtype).type
    n = A.shape[0]
    order, s = expected_method(norm1_f64(A))
    C = [R(c) for c in PADE[order]]
    As = A * R(2.0 ** -s)
    I = np.eye(n, dtype=T)
    A2 = As @ As
    P, U, V = I, C[1] * I, C[0] * I
    for j in range(1, len(C) // 2):
        P = P @ A2
        U = U + C[2 * j + 1] * P
        V = V + C[2 * j] * P
    U = As @ U
    D = V - U
    X = sl.lu_solve(sl.lu_factor(D, check_finite=False), V + U, check_finite=False)
    for _ in range(s):
        X = X @ X
    assert X.dtype == T and D.dtype == T
    return X, D, order, s


def exchange_stats(D):
    """LAPACK's partial pivoting (getrf) on D: exchanges, rows exchanged more than once, exchanges that leave their panel of the
    blocked LU, exchanges over at least PANEL_THREADS rows"""
    _, piv = sl.lu_factor(D, check_finite=False)
    n = len(piv)
    where = np.arange(n)                         # where[r]: the original row now stored in row r
    times = np.zeros(n, dtype=np.int64)
    out = dict(exchanges=0, rows_twice=0, leaving_panel=0, far=0)
    for c in range(n):
        p = int(piv[c])
        if p == c:
            continue
        out["exchanges"] += 1
        out["leaving_panel"] += int(p // LU_NB != c // LU_NB)
        out["far"] += int(p - c >= PANEL_THREADS)
        times[where[c]] += 1
        times[where[p]] += 1
        where[c], where[p] = where[p], where[c]
    out["rows_twice"] = int(np.sum(times > 1))
    return out


def pivot_gap(D):
    """Smallest (pivot - runner-up) / pivot over the columns of an unblocked elimination with partial pivoting in double precision
    (weights |x|, |re| + |im| for complex: what LAPACK's i?amax compares).  A step touches only the rows with a non-zero multiplier
    and the columns where the pivot row is non-zero; the others are left as they are, as the full rank-1 update would leave them."""
    M = np.array(D, dtype=np.complex128 if np.dtype(D.dtype).kind == "c" else np.float64, order="F")
    n = M.shape[0]
    gap = 1.0
    for c in range(n - 1):
        col = M[c:, c]
        w = np.abs(col.real) + np.abs(col.imag) if M.dtype.kind == "c" else np.abs(col)
        p = int(np.argmax(w))
        best = float(w[p])
        assert best > 0.0, "zero pivot column"
        w[p] = -1.0
        gap = min(gap, (best - float(np.max(w))) / best)
        if p != 0:
            M[[c, c + p], :] = M[[c + p, c], :]
        rows = c + 1 + np.flatnonzero(M[c + 1:, c])
        if len(rows):
            cols = c + 1 + np.flatnonzero(M[c, c + 1:])
            l = M[rows, c] / M[c, c]
            M[rows, c] = l
            if len(cols):
                M[np.ix_(rows, cols)] -= np.outer(l, M[c, cols])
    return gap


@functools.lru_cache(maxsize=None)
def skew_case(tname, n, k, norm1, with_gap=True):
    """Everything the tests need of one scattered-block case, computed once: A, the block reference, the restatement's result and
    error, LAPACK's exchange statistics on the CPU-formed V - U, the pivot gap (None when not asked for)"""
    A, blocks = scattered_skew(tname, n, k, norm1, 7 + n)
    ref = block_reference(A, blocks)
    E, D, order, s = restatement(A)
    return dict(A=A, blocks=blocks, ref=ref, restated=E, restated_err=rel_err(E, ref), D=D, order=order, s=s, norm1=norm1_f64(A),
                stats=exchange_stats(D), gap=pivot_gap(D) if with_gap else None)


# ------------------------------------------------------------------------------------------- thresholds of the method selection
def threshold_matrix(T, n, value, imaginary=False):
    """n x n matrix whose 1-norm is exactly |value| as stored: column n // 2 holds the single entry `value` (times i for
    `imaginary`; off the diagonal for n > 1), every other column sums to less than |value| / 64.  Complex matrices have purely real
    or purely imaginary entries, so every magnitude is exact."""
    T = np.dtype(T)
    rng = np.random.default_rng(n)
    A = rng.uniform(-1.0, 1.0, (n, n))
    A *= abs(float(value)) / (128.0 * np.abs(A).sum(axis=0).max())
    if T.kind == "c":
        A = np.where(rng.integers(0, 2, (n, n)) == 1, 1j * A, A + 0j)
    j = n // 2
    A[:, j] = 0
    A[(j + 1) % n, j] = (1j if imaginary else 1) * value
    A = np.asfortranarray(A.astype(T))
    return A


# ------------------------------------------------------------------------------------------- a column that needs fp64 sums
def f32_sums(c):
    """float32 sums of a float32 column in the orders an accumulation on the device could take: numpy's pairwise sum, the running
    sum, 256 strided partial sums folded by halving, and 16-byte packs (4 values per thread) folded the same way"""
    c = np.asarray(c, dtype=np.float32)

    def fold(part):
        part = np.concatenate([part, np.zeros(256 - len(part), dtype=np.float32)]) if len(part) < 256 else part
        w = 128
        while w > 0:
            part = (part[:w] + part[w:2 * w]).astype(np.float32)
            w //= 2
        return float(part[0])

    strided = np.array([np.cumsum(c[t::256], dtype=np.float32)[-1] if t < len(c) else 0 for t in range(256)], dtype=np.float32)
    packs = [c[4 * i:4 * i + 4] for i in range((len(c) + 3) // 4)]
    per_thread = np.zeros(256, dtype=np.float32)
    for i, pk in enumerate(packs):
        per_thread[i % 256] = np.float32(per_thread[i % 256] + np.cumsum(pk, dtype=np.float32)[-1])
    return dict(pairwise=float(np.sum(c, dtype=np.float32)), running=float(np.cumsum(c, dtype=np.float32)[-1]), strided=fold(strided),
                packed=fold(per_thread), packed_then_f64=float(np.sum(per_thread.astype(np.float64))))


def fp64_norm_column(n, seed, target=0.25, window=2e-10):
    """n positive float32 values whose double-precision sum lies in (target, target + window]: uniform(0.5, 1.5) draws scaled to
    the target, then single entries moved by one ulp until the sum is inside"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.5, 1.5, n)
    c = (u * (target / u.sum())).astype(np.float32)
    i = 0
    for _ in range(100000):
        s = float(np.sum(c.astype(np.float64)))
        if target < s <= target + window:
            return c
        c[i % n] = np.nextafter(c[i % n], np.float32(2.0 if s <= target else 0.0))
        i += 1
    raise AssertionError("no column found")


FP64_NORM_SEED = 2


def fp64_norm_matrix(n=300, seed=None):
    """(float32 matrix, index of the special column): that column is fp64_norm_column, every other one sums to 0.1"""
    seed = FP64_NORM_SEED if seed is None else seed
    rng = np.random.default_rng(1000 + seed)
    A = rng.uniform(0.5, 1.5, (n, n))
    A *= 0.1 / A.sum(axis=0)
    A = A.astype(np.float32)
    j = n // 3
    A[:, j] = fp64_norm_column(n, seed)
    return np.asfortranarray(A), j


# ------------------------------------------------------------------------------------------- the product, in more digits
def wide_product(alpha, A, B, beta, C0):
    """alpha A B + beta C0 accumulated one outer product per k in the next wider type (double for the 32-bit types, long double for
    the 64-bit ones; no BLAS), and |alpha| |A| |B| + |beta| |C0|, the scale of the componentwise error bound"""
    T = np.dtype(A.dtype)
    wide = {"f4": np.float64, "c8": np.complex128, "f8": np.longdouble, "c16": np.clongdouble}[T.kind + str(T.itemsize)]
    Aw, Bw = A.astype(wide), B.astype(wide)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=wide)
    mag = np.zeros(acc.shape, dtype=np.float64)
    aA, aB = np.abs(A).astype(np.float64), np.abs(B).astype(np.float64)
    for kk in range(A.shape[1]):
        acc += np.outer(Aw[:, kk], Bw[kk, :])
        mag += np.outer(aA[:, kk], aB[kk, :])
    return wide(alpha) * acc + wide(beta) * C0.astype(wide), abs(alpha) * mag + abs(beta) * np.abs(C0).astype(np.float64)


def product_gamma(T, k):
    """gamma of |C^ - C| <= gamma (|alpha| |A| |B| + |beta| |C0|) for EVERY summation order, u = eps / 2: (k + 2) u for the real
    types (k products and k additions along any tree, the scaling by beta and the final addition), 2 sqrt(2) (k + 4) u for the
    complex ones (a complex product carries 2 sqrt(2) u instead of u)"""
    T = np.dtype(T)
    u = float(np.finfo(real_type(T)).eps) / 2
    return 2 * math.sqrt(2) * (k + 4) * u if T.kind == "c" else (k + 2) * u


# ------------------------------------------------------------------------------------------- exactly tied pivot candidates
TIED_A_RANGE = (1.95, 2.15)


def tied_hubs(T, n, seed):
    """(A, blocks): 3 x 3 skew blocks a [[0, -1, -1], [1, 0, 0], [1, 0, 0]] (complex types: i a [[0, 1, 1], [1, 0, 0], [1, 0, 0]])
    on rows h < l1 < l2 scattered over [0, n), a drawn from TIED_A_RANGE per block; the n mod 3 rows left over are zero.

    Rows l1 and l2 of A are equal, so they are equal bit for bit in every product X Y with X = A, A^2 or a power of it whenever an
    entry's sum over k runs in an order that does not depend on its row: column h of V - U holds the SAME value in rows l1 and l2.
    With x = a / sqrt(2) in (1.38, 1.52), V - U ~ c exp(-A / 2) has there |cos x| on the diagonal and sin x / sqrt(2), three times
    larger, in both rows: an exact tie that LAPACK's rule (the first maximal entry) gives to l1.  The block's second pivot is then
    decided between cot(x / 2) / sqrt(2) < 0.9 in row l1 and 1 in row l2: a second exchange.  Taking l2 in the tie leaves
    1 in row l1 against tan(x / 2) / sqrt(2) < 0.72: no second exchange.  Two exchanges per block against one, and no other
    candidate within 10 % of a pivot (tied_block_exchanges measures both)."""
    T = np.dtype(T)
    rng = np.random.default_rng(seed)
    p = rng.permutation(n)
    A = np.zeros((n, n), dtype=np.complex128 if T.kind == "c" else np.float64)
    blocks = []
    for q in range(0, n - 2, 3):
        h, l1, l2 = sorted(int(v) for v in p[q:q + 3])
        a = rng.uniform(*TIED_A_RANGE)
        if T.kind == "c":
            A[[l1, l2], h] = 1j * a
            A[h, [l1, l2]] = 1j * a
        else:
            A[[l1, l2], h] = a
            A[h, [l1, l2]] = -a
        blocks.append(np.array([h, l1, l2]))
    single = [np.array([int(r)]) for r in p[3 * len(blocks):]]
    A = np.asfortranarray(A.astype(T))
    A.setflags(write=False)
    return A, blocks, single


def tied_block_exchanges(D, blocks, last, tie_tol):
    """Partial pivoting inside every 3 x 3 block of the block-scattered D (the rows of a block are ascending, so this IS the
    elimination of the whole matrix), candidates within tie_tol (relative) of the largest counted as tied and the first (`last`: the
    last) of them taken.  Returns (exchanges, tied columns, smallest relative gap between the tied group and the other candidates)."""
    count, tied, gap = 0, 0, 1.0
    for idx in blocks:
        M = np.array(D[np.ix_(idx, idx)], dtype=np.complex128)
        for c in range(len(idx) - 1):
            w = np.abs(M[c:, c].real) + np.abs(M[c:, c].imag)
            group = np.flatnonzero(w >= w.max() * (1 - tie_tol))
            tied += int(len(group) > 1)
            others = np.delete(w, group)
            if len(others):
                gap = min(gap, float((w.max() - others.max()) / w.max()))
            p = int(group[-1] if last else group[0])
            if p:
                M[[c, c + p]] = M[[c + p, c]]
                count += 1
            M[c + 1:, c] /= M[c, c]
            M[c + 1:, c + 1:] -= np.outer(M[c + 1:, c], M[c, c + 1:])
    return count, tied, gap


@functools.lru_cache(maxsize=None)
def tied_case(tname, n):
    A, blocks, single = tied_hubs(tname, n, 11 + n)
    ref = block_reference(A, blocks + single)
    E, D, order, s = restatement(A)
    tol = 64 * float(np.finfo(np.dtype(tname)).eps)
    return dict(A=A, blocks=blocks, ref=ref, restated_err=rel_err(E, ref), D=D, order=order, s=s, norm1=norm1_f64(A),
                first=tied_block_exchanges(D, blocks, False, tol), last=tied_block_exchanges(D, blocks, True, tol))
