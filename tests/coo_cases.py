"""Coordinate triplets for the tests of expv_mi_op_create_coo_loc, and the CPU side of its contract; no device work here.

The library's operator is that of the matrix a_ij = sum of the entries with coordinates (i, j), summed in the element type in
ascending order of the entry's position.  `expected_csr` is that definition in numpy: a stable lexsort by (row, col), then
np.add.at, which adds one entry after the other.  Two ways of turning a matrix into triplets with repeats:

  exact    v -> (v/4, v/4, v/2) or (v/2, v/2), the pieces kept in this order among the shuffled triplets.  v/4 + v/4 = v/2 and
           v/2 + v/2 = v are exact, so the expected matrix IS the original one (the intermediate 3v/4 of another order need not be).
  random   v -> (v, p, q) with unrelated p, q: compared with expected_csr.
"""
import numpy as np
import scipy.sparse as sp


def expected_csr(row, col, vals, n):
    """the CSR matrix the contract defines for these zero-based triplets (stored zeros kept)"""
    row, col, vals = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(vals)
    order = np.lexsort((col, row))                       # stable: equal coordinates keep their entry order
    r, c, v = row[order], col[order], vals[order]
    head = np.ones(len(r), dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    cell = np.cumsum(head) - 1
    nst = int(head.sum())
    data = np.zeros(nst, dtype=vals.dtype)
    np.add.at(data, cell, v)                             # one entry after the other, in the element type
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, r[head] + 1, 1)
    return sp.csr_matrix((data, c[head].astype(np.int32), np.cumsum(indptr).astype(np.int32)), shape=(n, n))


def _shuffle_keeping_piece_order(group, rng):
    """a random order of the triplets in which the pieces of one group (laid out contiguously, in piece order) keep their order"""
    keys = rng.random(len(group))
    keys = keys[np.lexsort((keys, group))]               # inside every group the keys now ascend with the piece number
    return np.argsort(keys, kind="stable")


def split_triplets(A, share, mode, seed):
    """(row, col, vals) of the sorted CSR matrix A, shuffled, with `share` of its entries split into repeats (mode "exact" / "random")"""
    A = A.tocsr()
    A.sort_indices()
    rng = np.random.default_rng(seed)
    C = A.tocoo()
    nnz = C.nnz
    pieces = np.ones(nnz, dtype=np.int64)
    chosen = rng.random(nnz) < share
    pieces[chosen] = 2 + (rng.random(int(chosen.sum())) < 0.5)
    group = np.repeat(np.arange(nnz), pieces)
    first = np.concatenate([[0], np.cumsum(pieces)[:-1]])
    j = np.arange(len(group)) - first[group]              # piece number inside the entry
    v = C.data[group].copy()
    if mode == "exact":
        v[(pieces[group] == 2)] = C.data[group][pieces[group] == 2] / 2
        three = pieces[group] == 3
        v[three & (j < 2)] = C.data[group][three & (j < 2)] / 4
        v[three & (j == 2)] = C.data[group][three & (j == 2)] / 2
    else:
        extra = j > 0
        noise = rng.standard_normal(int(extra.sum()))
        if np.iscomplexobj(v):
            noise = noise + 1j * rng.standard_normal(int(extra.sum()))
        v[extra] = noise.astype(v.dtype)
    perm = _shuffle_keeping_piece_order(group, rng)
    return C.row[group][perm].astype(np.int64), C.col[group][perm].astype(np.int64), np.ascontiguousarray(v[perm])


def random_triplets(n, count, T, seed, repeat_share=0.1, lo=0, hi=None, ends=False):
    """`count` triplets with rows and columns in [lo, hi), ~repeat_share of them repeating an earlier coordinate; ends: the first two
    are (0, 0) and (n - 1, n - 1)"""
    rng = np.random.default_rng(seed)
    hi = n if hi is None else hi
    row, col = rng.integers(lo, hi, count), rng.integers(lo, hi, count)
    rep = np.flatnonzero(rng.random(count) < repeat_share)
    rep = rep[rep > 0]
    src = (rng.random(len(rep)) * rep).astype(np.int64)      # an earlier position
    row[rep], col[rep] = row[src], col[src]
    if ends and count >= 2:
        row[0] = col[0] = 0
        row[1] = col[1] = n - 1
    v = rng.standard_normal(count)
    if np.dtype(T).kind == "c":
        v = v + 1j * rng.standard_normal(count)
    return row.astype(np.int64), col.astype(np.int64), v.astype(T)
