"""Inputs of the adjoint / transpose operator tests and the CPU restatement of its definition (no device work here).

expv_mi_op_create_adjoint is DEFINED as the operator expv_mi_op_create_csr_loc makes of the zero-based CSR arrays of A' (or
transpose(A)) in the natural ordering with every row in ascending column order.  `adjoint_arrays` states those arrays in numpy,
together with the source map the library keeps for its refresh; tests/test_adjoint_cpu.py holds it against scipy.

The generators are integer-valued (entries, real and imaginary parts in {-3 ... 3}, some of them stored zeros), so that products
with integer vectors are exact in every element type and the adjoint identity <y, A x> = <A' y, x> can be asserted without a
tolerance."""
import numpy as np
import scipy.sparse as sp

DTYPES = [np.float64, np.complex128, np.float32, np.complex64]


def adjoint_arrays(rp, ci, va, conj):
    """(rowptr, colind, vals, src) of A' (conj) / transpose(A) of the CSR arrays rp, ci, va: entry e of the result is entry
    src[e] of the input, rows ascending, columns ascending inside a row, entries of one coordinate in input order (a stable
    sort).  Repeated coordinates stay separate entries; stored zeros stay stored."""
    rp, ci, va = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(va)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    src = np.lexsort((rows, ci))      # (stable: primary key the input column = the new row, then the input row = the new column)
    rp2 = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=rp2[1:])
    v2 = va[src]
    if conj:
        v2 = np.conj(v2)
    return rp2.astype(np.int32), rows[src].astype(np.int32), np.ascontiguousarray(v2), src.astype(np.int32)


def int_values(count, T, rng, zero_share=0.1):
    """`count` values of type T with integer parts in {-3 ... 3}; about zero_share of them are (stored) zeros"""
    v = rng.integers(-3, 4, count).astype(np.float64)
    if np.dtype(T).kind == "c":
        v = v + 1j * rng.integers(-3, 4, count)
    v[rng.random(count) < zero_share] = 0
    return v.astype(T)


def _csr(n, rows, cols, T, rng):
    """the CSR matrix of the distinct coordinates with integer values; stored zeros are kept"""
    keys = np.unique(np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64))
    r, c = keys // n, keys % n
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    A = sp.csr_matrix((int_values(len(keys), T, rng), c.astype(np.int32), rp.astype(np.int32)), shape=(n, n))
    A.has_sorted_indices = True
    return A


def band(n, T, seed=1, offsets=(-3, -1, 0, 2, 5)):
    """a band with an unsymmetric set of offsets"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    rows = np.concatenate([i[(i + k >= 0) & (i + k < n)] for k in offsets])
    cols = np.concatenate([i[(i + k >= 0) & (i + k < n)] + k for k in offsets])
    return _csr(n, rows, cols, T, rng)


def upper(n, T, seed=2, per_row=6):
    """the shape of the reference's GPU test matrix: a random strictly upper triangle and a few entries anywhere"""
    rng = np.random.default_rng(seed)
    m = per_row * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = r < c
    extra = max(1, n // 8)
    rows = np.concatenate([r[keep], rng.integers(0, n, extra)])
    cols = np.concatenate([c[keep], rng.integers(0, n, extra)])
    return _csr(n, rows, cols, T, rng)


def unequal_rows(n, T, seed=3):
    """rows of very unequal length: a few full rows, a few empty ones, a diagonal, one dense column"""
    rng = np.random.default_rng(seed)
    full = np.unique(rng.integers(0, n, max(1, n // 40)))
    rows = [np.repeat(full, n), np.arange(n), np.arange(n)]
    cols = [np.tile(np.arange(n), len(full)), np.arange(n), np.full(n, n // 3)]
    A = _csr(n, np.concatenate(rows), np.concatenate(cols), T, rng).tolil()
    for e in np.unique(rng.integers(0, n, max(1, n // 10))):      # empty rows (not the full ones)
        if e not in full:
            A.rows[e], A.data[e] = [], []
    A = A.tocsr()
    A.sort_indices()
    return A


CASES = {"band": band, "upper": upper, "unequal_rows": unequal_rows}


def int_vector(n, T, seed):
    """entries (and imaginary parts) in {-2 ... 2}"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, n).astype(np.float64)
    if np.dtype(T).kind == "c":
        x = x + 1j * rng.integers(-2, 3, n)
    return x.astype(T)


def with_repeat(A, seed=4):
    """CSR arrays of A with one row's first two entries swapped and its first coordinate stored twice more (values split so that
    the matrix is unchanged where the values are integers): unsorted rows with a repeated coordinate"""
    A = A.tocsr()
    A.sort_indices()
    r = int(np.argmax(np.diff(A.indptr) >= 2))
    k = int(A.indptr[r])
    ip, ix, va = A.indptr.astype(np.int64), A.indices.copy(), A.data.copy()
    ix[[k, k + 1]] = ix[[k + 1, k]]
    va[[k, k + 1]] = va[[k + 1, k]]
    # the coordinate now at k again at the end of the row: value 1 there, the original lowered by 1
    end = int(ip[r + 1])
    ix = np.insert(ix, end, ix[k])
    va = np.insert(va, end, 1)
    va[k] -= 1
    ip[r + 1:] += 1
    return ip.astype(np.int32), ix.astype(np.int32), va
