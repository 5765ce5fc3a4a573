"""Operators for the constant-tile mask of the banded Float64 form (context option "elide") and the rule itself, restated in numpy.
No device work here: tests/test_elide_mask_rule.py checks the restatement, tests/test_gpu_elide_const_tiles.py the library against it.

The rule (csrc/kernels.hip, k_op_dia_const): the banded form stores diagonal d of row r at dia[d, r], r < ld = n rounded up to 512,
with +0.0 wherever the matrix has no entry (rows whose column r + offset lies outside, rows >= n).  Bit d of mask[t] is set when all
512 STORED entries dia[d, 512 t : 512 t + 512] carry one bit pattern and none is a NaN.  So the first tile of every sub-diagonal and
the last tile of every diagonal of a matrix whose n is no multiple of 512 are "not constant" through the zero fill alone (n a multiple
of 512: the last tile of every super-diagonal), unless the diagonal's own value there is +0.0."""
import numpy as np
import scipy.sparse as sp

from tests._util import C2_OFFSETS, C2_SYM_VALS, C2_VALS

TILE = 512
N_SMALL = 3 * TILE + 37          # 4 tiles, the last one ragged
N_EVEN = 4 * TILE                # 4 whole tiles: the zero fill of the super-diagonals sits inside the last one


def csr_from_diagonals(n, offsets, diags):
    """CSR matrix with EVERY in-matrix position of the given diagonals stored, explicit zeros (and their signs) included; diags[d][k] is
    the entry in row max(0, -o) + k of diagonal o = offsets[d]"""
    rows, cols, vals = [], [], []
    for o, v in zip(offsets, diags):
        r = np.arange(max(0, -o), min(n, n - o))
        assert len(v) == len(r), (o, len(v), len(r))
        rows.append(r)
        cols.append(r + o)
        vals.append(np.asarray(v, dtype=np.float64))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sort_indices()
    assert A.nnz == sum(len(v) for v in vals)      # (nothing dropped)
    return A


def stored_diagonals(A, offsets):
    """the [ndiag][ld] array of the banded form: entry (r, r + o) at [d, r], +0.0 elsewhere"""
    n = A.shape[0]
    ld = (n + TILE - 1) // TILE * TILE
    out = np.zeros((len(offsets), ld))
    A = A.tocsr()
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    order = {o: d for d, o in enumerate(offsets)}
    d = np.array([order[int(o)] for o in (A.indices - rows)])
    out[d, rows] = A.data
    return out


def tile_mask(stored):
    """mask[t] bit d <=> diagonal d holds one bit pattern, no NaN, on stored rows 512 t .. 512 t + 511"""
    nd, ld = stored.shape
    bits = stored.view(np.uint64).reshape(nd, ld // TILE, TILE)
    same = (bits == bits[:, :, :1]).all(axis=2) & ~np.isnan(stored.reshape(nd, ld // TILE, TILE)).any(axis=2)
    return (same * (1 << np.arange(nd))[:, None]).sum(axis=0).astype(np.uint8)


def _diags(n, vals):
    return [np.full(n - abs(o), v) for o, v in zip(C2_OFFSETS, vals)]


def case(name, n=N_SMALL, sym=False):
    """(a) five constant diagonals; (b) = (a) with one interior entry of the main diagonal changed; (c) the first super-diagonal changes
    its value exactly at a tile boundary (sym: the first sub-diagonal with it, so the matrix stays symmetric); (d) the second
    super-diagonal is +0.0 with one -0.0; (e) random; (nan) = (a) with one NaN on the main diagonal.  Same pattern for all."""
    vals = C2_SYM_VALS if sym else C2_VALS
    D = _diags(n, vals)
    if name == "b":
        D[2][700] = vals[2] - 0.25
    elif name == "c":
        D[3][2 * TILE:] = 0.7                      # rows >= 1024 of offset +1
        if sym:
            D[1][2 * TILE:] = 0.7                  # entry (r + 1, r), r >= 1024: stored at row r + 1 of offset -1
    elif name == "d":
        assert not sym
        D[4][:] = 0.0
        D[4][600] = -0.0
    elif name == "e":
        rng = np.random.default_rng(11)
        D = [0.3 * rng.standard_normal(len(v)) - (2.0 if o == 0 else 0.0) for o, v in zip(C2_OFFSETS, D)]
        if sym:
            D[0], D[1] = D[4].copy(), D[3].copy()
    elif name == "nan":
        D[2][900] = np.nan
    else:
        assert name == "a", name
    return csr_from_diagonals(n, C2_OFFSETS, D)


def tenth_perturbed(n, seed=5):
    """C2 with one entry of the main diagonal changed in a tenth of the tiles (every tenth tile)"""
    D = _diags(n, C2_VALS)
    for t in range(3, (n + TILE - 1) // TILE - 1, 10):
        D[2][t * TILE + 100] = -2.5
    return csr_from_diagonals(n, C2_OFFSETS, D)


# constant (tile, diagonal) pairs of the cases at N_SMALL, worked out by hand from the rule: main diagonal tiles 0..2; sub-diagonals
# tiles 1, 2 (tile 0 starts with zero fill); super-diagonals tiles 0..2; nobody's tile 3 (rows >= n are zero fill)
EXPECTED_PAIRS = {"a": 13, "b": 12, "c": 13, "d": 13, "e": 0, "nan": 12}
# (d): the +0.0 super-diagonal is constant on tiles 0, 2 and -- zero fill and value being the same bits -- 3; tile 1 holds the -0.0
