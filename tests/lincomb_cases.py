"""Inputs of the linear-combination operator tests and the CPU restatement of its definition (no device work here).

expv_mi_op_create_lincomb is DEFINED as the operator expv_mi_op_create_csr_loc makes of the zero-based CSR arrays of
c_1 A_1 + ... + c_K A_K (+ c_I I): the pattern is the union of the terms' coordinates (plus the diagonal with the identity), rows
sorted and free of repeats, whatever the values are; the contributions to one coordinate are added left to right in term order,
inside a term that repeats a coordinate in its stored order, the identity last; the accumulator starts as the first contribution;
a coefficient with a zero imaginary part multiplies each real component once, a complex one gives (cr ar - ci ai, cr ai + ci ar)
with every product rounded before the sum or difference; the identity contributes its coefficient as it is.  `lincomb_arrays`
states that in numpy on real and imaginary parts (numpy's complex multiply is not used: its kernels may fuse);
tests/test_lincomb_cpu.py holds it against scipy.

A term is a triple (rowptr, colind, vals) of CSR arrays in the natural ordering; its rows need not be sorted and may repeat a
coordinate.  The generators are those of tests/adjoint_cases.py: integer-valued, some entries stored zeros."""
import numpy as np
import scipy.sparse as sp

from tests import adjoint_cases as ac

DTYPES = ac.DTYPES


def real_type(T):
    return np.float32 if np.dtype(T) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def scaled(c, v):
    """c v under the contract: c a Python scalar, rounded once to the real type of v's element type; v an array"""
    T = v.dtype
    R = real_type(T)
    c = complex(c)
    cr, ci = R(c.real), R(c.imag)
    if T.kind != "c":
        assert ci == 0
        return (cr * v).astype(T)
    ar, ai = np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
    out = np.empty(v.shape, dtype=T)
    if ci == 0:
        out.real, out.imag = cr * ar, cr * ai
    else:
        p1, p2, p3, p4 = cr * ar, ci * ai, cr * ai, ci * ar      # (four rounded products, then one rounded sum or difference each)
        out.real, out.imag = p1 - p2, p3 + p4
    return out


def lincomb_arrays(terms, coefs, identity=None):
    """(rowptr, colind, vals) of coefs[0] terms[0] + ... (+ identity I) under the contract above.  terms: (rowptr, colind, vals)
    triples of one size and element type."""
    assert len(terms) == len(coefs) and len(terms) >= 1
    T = np.asarray(terms[0][2]).dtype
    n = len(terms[0][0]) - 1
    rows, cols, contrib = [], [], []
    for (rp, ci, va), c in zip(terms, coefs):
        rp, ci, va = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64), np.asarray(va)
        assert len(rp) == n + 1 and va.dtype == T
        rows.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)))
        cols.append(ci)
        contrib.append(scaled(c, va))
    if identity is not None:
        R = real_type(T)
        c = complex(identity)
        d = np.arange(n, dtype=np.int64)
        rows.append(d)
        cols.append(d)
        contrib.append(np.full(n, R(c.real) + 1j * R(c.imag) if T.kind == "c" else R(c.real), dtype=T))
    rows, cols, contrib = np.concatenate(rows), np.concatenate(cols), np.concatenate(contrib)
    key = rows * max(n, 1) + cols
    order = np.argsort(key, kind="stable")      # positions of one coordinate stay in the order of the concatenation
    key, contrib = key[order], contrib[order]
    total = len(key)
    head = np.ones(total, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, total))
    vals = contrib[start].copy()                # the accumulator starts as the first contribution
    for d in range(1, int(length.max()) if total else 0):
        more = length > d
        vals[more] = vals[more] + contrib[start[more] + d]      # (componentwise additions, left to right)
    ukey = key[start]
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ukey // max(n, 1), minlength=n), out=rp[1:])
    return rp.astype(np.int32), (ukey % max(n, 1)).astype(np.int32), np.ascontiguousarray(vals)


def arrays(A):
    """the term of a scipy matrix: sorted rows"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data)


def matrix(term):
    """the scipy matrix of a term (repeated coordinates summed by scipy)"""
    rp, ci, va = term
    n = len(rp) - 1
    return sp.csr_matrix((va, ci, rp), shape=(n, n))


# ---- the cases: n, T -> list of terms ---------------------------------------------------------------------------------------------
OFFSETS_A, OFFSETS_B = (-3, -1, 0, 2, 5), (-6, -2, 0, 1, 4)


def two_bands(n, T):
    """two bands with different offsets (they share the diagonal)"""
    return [arrays(ac.band(n, T, 1, OFFSETS_A)), arrays(ac.band(n, T, 7, OFFSETS_B))]


def same_pattern(n, T):
    """two operators of one pattern, other values"""
    return [arrays(ac.band(n, T, 1, OFFSETS_A)), arrays(ac.band(n, T, 8, OFFSETS_A))]


def disjoint(n, T):
    """strictly upper plus strictly lower"""
    U = sp.triu(ac.upper(n, T, 2), 1, format="csr")
    Lo = sp.tril(ac.upper(n, T, 5).T.tocsr(), -1, format="csr")
    return [arrays(U.astype(T)), arrays(Lo.astype(T))]


def empty_rows(n, T):
    """a term with empty rows (and a few full ones) and a band"""
    return [arrays(ac.unequal_rows(n, T)), arrays(ac.band(n, T, 1, OFFSETS_B))]


def zero_term(n, T):
    """the zero operator as a term"""
    return [arrays(ac.band(n, T, 3, OFFSETS_A)), arrays(sp.csr_matrix((n, n), dtype=T))]


def own_adjoint(n, T):
    """one term and its own adjoint (the second term is the restatement's adjoint of the first)"""
    a = arrays(ac.upper(n, T, 6))
    rp, ci, va, _ = ac.adjoint_arrays(*a, True)
    return [a, (rp, ci, va)]


def repeated(n, T):
    """a term whose rows repeat a coordinate (unsorted, too) and a band"""
    if n < 2:
        rep = (np.array([0, 3], dtype=np.int32), np.zeros(3, dtype=np.int32), np.array([2, -0.0, 1]).astype(T))
    else:
        rep = ac.with_repeat(ac.band(n, T, 4, OFFSETS_A))
        rep = (rep[0], rep[1], np.ascontiguousarray(rep[2]).astype(T))
    return [rep, arrays(ac.band(n, T, 9, OFFSETS_B))]


def eight_terms(n, T):
    """the cap: 8 terms, bands of two patterns in turn"""
    return [arrays(ac.band(n, T, 20 + k, OFFSETS_A if k % 2 == 0 else OFFSETS_B)) for k in range(8)]


CASES = {"two_bands": two_bands, "same_pattern": same_pattern, "disjoint": disjoint, "empty_rows": empty_rows, "zero_term": zero_term,
         "own_adjoint": own_adjoint, "repeated": repeated, "eight_terms": eight_terms}

REAL_COEFS = [2.0, -1.0, 0.5, -3.0, 1.0, 0.0, 1.5, -0.25]
COMPLEX_COEFS = [1.0 + 2.0j, -1.0, 0.5 - 1.0j, -3.0j, 2.0, 0.0, 1.5 + 0.5j, -0.25]


def coefficient_sets(K, T):
    """[(coefs, identity)]: real with negatives and a zero; with the identity; for the complex types complex ones, with a complex identity"""
    sets = [(REAL_COEFS[:K], None), ([-c for c in REAL_COEFS[:K]], -2.0)]
    if np.dtype(T).kind == "c":
        sets += [(COMPLEX_COEFS[:K], None), (COMPLEX_COEFS[:K][::-1], 0.5 + 1.0j)]
    return sets
