"""Block-compressed (BSR / BSC) test inputs and the position contract of expv_mi_op_create_bsr_loc restated in numpy.

`expand` is the contract of include/expv_mi.h, nothing else: block k = ptr[b] + kk of compressed block row (column) b with
cnt = ptr[b + 1] - ptr[b] puts its element with outer in-block index o and inner in-block index i at scalar position
bd^2 ptr[b] + o bd cnt + kk bd + i, scalar index idx[k] bd + i, scalar pointer [b bd + o] = bd^2 ptr[b] + o bd cnt.  For BSR
(o, i) = (row, column) inside the block, for BSC (column, row).  tests/test_bsr_operator_cpu.py holds it against scipy."""
import numpy as np
import scipy.sparse as sp


def expand(ptr, idx, vals, bd, block_order="row", compressed="rows", index_base=0):
    """(sptr[n + 1], sidx[nnz], sval[nnz]): the scalar CSR (compressed="rows") or CSC ("cols") arrays, zero-based int64 / the
    dtype of vals.  vals[k] holds block k row-major (block_order="row": vals[k][r][c]) or column-major ("col": vals[k][c][r])."""
    ptr = np.asarray(ptr, dtype=np.int64) - index_base
    idx = np.asarray(idx, dtype=np.int64) - index_base
    vals = np.asarray(vals).reshape(len(idx), bd, bd)
    nb, nnzb = len(ptr) - 1, len(idx)
    cnt = np.diff(ptr)
    b = np.repeat(np.arange(nb), cnt)                      # compressed block row (column) of block k
    kk = np.arange(nnzb) - ptr[b]
    o, i = np.arange(bd)[None, :, None], np.arange(bd)[None, None, :]
    pos = (bd * bd * ptr[b] + kk * bd)[:, None, None] + o * (bd * cnt[b])[:, None, None] + i
    outer_major = (block_order == "row") == (compressed == "rows")
    V = vals if outer_major else vals.transpose(0, 2, 1)    # V[k][o][i]
    sval = np.empty(nnzb * bd * bd, dtype=vals.dtype)
    sidx = np.empty(nnzb * bd * bd, dtype=np.int64)
    sval[pos.ravel()] = V.ravel()
    sidx[pos.ravel()] = np.broadcast_to((idx * bd)[:, None, None] + i, pos.shape).ravel()
    sptr = np.empty(nb * bd + 1, dtype=np.int64)
    sptr[:-1] = ((bd * bd * ptr[:-1])[:, None] + np.arange(bd)[None, :] * (bd * cnt)[:, None]).ravel()
    sptr[-1] = nnzb * bd * bd
    return sptr, sidx, sval


def scalar_matrix(ptr, idx, vals, bd, block_order="row", compressed="rows", index_base=0):
    """the scalar scipy matrix (csr_matrix / csc_matrix) of `expand`'s arrays, entry order kept"""
    sptr, sidx, sval = expand(ptr, idx, vals, bd, block_order, compressed, index_base)
    n = len(sptr) - 1
    mk = sp.csr_matrix if compressed == "rows" else sp.csc_matrix
    return mk((sval, sidx.astype(np.int32), sptr.astype(np.int32)), shape=(n, n))


def random_values(shape, T, rng):
    v = rng.standard_normal(shape)
    if np.dtype(T).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v.astype(T)


def from_block_pattern(P, bd, T, seed):
    """BSR arrays (ptr, idx, vals row-major) with random blocks on the block pattern P (a scipy sparse matrix, nb x nb), block
    rows sorted; int64 indices"""
    P = sp.csr_matrix(P)
    P.sort_indices()
    rng = np.random.default_rng(seed)
    return P.indptr.astype(np.int64), P.indices.astype(np.int64), random_values((P.nnz, bd, bd), T, rng)


def block_tridiagonal(nb, bd, T, seed=5):
    return from_block_pattern(sp.diags([np.ones(nb - 1), np.ones(nb), np.ones(nb - 1)], [-1, 0, 1]), bd, T, seed)


def with_empty_block_rows(nb, bd, T, seed=6, per_row=3):
    """empty block rows at the start, in two runs in the middle, and at the end; nb >= 16"""
    rng = np.random.default_rng(seed)
    P = sp.random(nb, nb, density=per_row / nb, random_state=rng, format="lil")
    for r in [0, 1, 5, 6, 7, 10, nb - 2, nb - 1]:
        P[r, :] = 0
    P[3, 0] = P[3, nb - 1] = 1.0            # ... while the first and the last block COLUMN are in use
    P = sp.csr_matrix(P)
    P.eliminate_zeros()
    return from_block_pattern(P, bd, T, seed)


def as_block_order(vals, block_order):
    """row-major blocks restated in the given order"""
    return vals if block_order == "row" else np.ascontiguousarray(vals.transpose(0, 2, 1))


def bsc_of(ptr, idx, vals, bd):
    """the BSC arrays (ptr over block columns, idx = block rows, row-major blocks) of the matrix whose sorted BSR arrays are given:
    through A.T as BSR, whose blocks are the transposes"""
    n = (len(ptr) - 1) * bd
    At = sp.bsr_matrix((vals, idx, ptr), shape=(n, n)).T.tobsr(blocksize=(bd, bd))
    At.sort_indices()
    assert At.data.shape[0] == len(idx)      # (no block lost: tobsr keeps stored zeros of a BSR transpose)
    return At.indptr.astype(np.int64), At.indices.astype(np.int64), np.ascontiguousarray(At.data.transpose(0, 2, 1))


def reverse_block_rows(ptr, idx, vals):
    """the same matrix with the blocks of every block row in reverse order"""
    order = np.concatenate([np.arange(ptr[b + 1] - 1, ptr[b] - 1, -1) for b in range(len(ptr) - 1)]).astype(np.int64) \
        if len(idx) else np.zeros(0, dtype=np.int64)
    return ptr, idx[order], vals[order]
