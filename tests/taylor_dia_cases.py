"""Operators for the truncated-Taylor entries (expv_taylor, expv_taylor_block, phiv_taylor, expv_taylor_grid) that reach the parts of
csrc/sparse_rows.h the operators of tests/expv_taylor_cases.py do not: the general diagonal form with its own array (more than
PIPE_DIA_MAX diagonals or a band wider than PIPE_WMAX, up to GDIA_MAX offsets), the column guard of dia_walk at offsets beyond a pack,
a slice and a 512-row unit of the array's leading dimension, every remainder of the in-flight loops (Q = 4 and Q = 2), explicit zeros of
the form inside a sum, and rows without a stored diagonal entry.  No device work here.

Values are of size ~ 1 / sqrt(nd) with a diagonal near -1, so that alpha = 40 gives several stages (tc.t_for)."""
import math

import numpy as np
import scipy.sparse as sp

from tests import expv_taylor_cases as tc
from tests import limits
from tests.limits import LIMITS
from tests.test_gpu_limits import OFFS_HB8_D8, OFFS_HB8_D9

DTYPES = tc.DTYPES


def slice_rows(T):
    """rows of a SELL slice of the element type: 64 lanes x one 16-byte pack"""
    return 64 * (16 // np.dtype(T).itemsize)


# ---- generators --------------------------------------------------------------------------------------------------------------
def _values(r, count, scale, T):
    v = r.standard_normal(count) * scale
    if np.dtype(T).kind == "c":
        v = v * np.exp(2j * np.pi * r.random(count))
    return v


def _main(r, count, T):
    d = -1.0 + 0.1 * r.standard_normal(count)
    if np.dtype(T).kind == "c":
        d = d + 0.1j * r.standard_normal(count)
    return d


def _csr(n, rows, cols, vals, T):
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A.astype(T).tocsr()


def diagonals(n, offsets, T, keep=1.0, drop=None, main_keep=1.0):
    """The operator with the distinct `offsets` (column - row), rows sorted.  keep < 1 removes that share of the off-diagonal entries at
    random rows (drop: that many of them exactly), main_keep < 1 of the main diagonal's: explicit zeros in a diagonal form.  The caller
    stays inside limits.fill_ok(nd, n, nnz) where it wants one."""
    offsets = tuple(int(o) for o in offsets)
    assert len(set(offsets)) == len(offsets) and all(abs(o) < n for o in offsets)
    nd = len(offsets)
    r = tc.rng_of(n, 144, nd, sum(abs(o) for o in offsets))
    rows, cols, vals = [], [], []
    for o in offsets:
        i = np.arange(max(0, -o), min(n, n - o))
        rows.append(i)
        cols.append(i + o)
        vals.append(_main(r, i.size, T) if o == 0 else _values(r, i.size, 1.0 / math.sqrt(nd), T))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    off = np.flatnonzero(rows != cols)
    main = np.flatnonzero(rows == cols)
    gone = int(round((1.0 - keep) * off.size)) if drop is None else int(drop)
    assert 0 <= gone <= off.size
    out = np.ones(rows.size, dtype=bool)
    out[r.permutation(off)[:gone]] = False
    out[r.permutation(main)[:int(round((1.0 - main_keep) * main.size))]] = False
    return _csr(n, [rows[out]], [cols[out]], [vals[out]], T)


def _stencil(n, T, offsets, neighbour, seed):
    """variable, non-symmetric coefficients on `offsets`; neighbour(i, o): the rows i whose cell i + o is a neighbour in the grid"""
    nd = len(offsets)
    r = tc.rng_of(n, 233, seed, nd)
    i = np.arange(n)
    rows, cols, vals = [], [], []
    for o in offsets:
        ok = (i + o >= 0) & (i + o < n) & neighbour(i, o)
        rows.append(i[ok])
        cols.append(i[ok] + o)
        if o == 0:
            vals.append(_main(r, int(ok.sum()), T))
        else:
            # another size on either side, and another sign for the neighbours in other grid rows: with a diagonal near -1 the result
            # neither decays nor grows by more than a few orders over alpha = 40, and its relative error means something
            c = (0.6 + 0.8 * r.random()) * (1.0 if o > 0 else (0.7 if o == -1 else -0.7)) / math.sqrt(nd)
            v = c * (1.0 + 0.3 * r.random(int(ok.sum())))
            vals.append(v * np.exp(0.9j * o / abs(o)) if np.dtype(T).kind == "c" else v)
    return _csr(n, rows, cols, vals, T)


def grid5(nx, ny, T, n=None):
    """5-point stencil on a grid with rows of nx cells, ny rows (n: only its first n cells -- the last grid row is incomplete);
    no coupling over the end of a grid row: the +-1 diagonals are absent there"""
    assert nx != ny
    n = nx * ny if n is None else n
    return _stencil(n, T, (-nx, -1, 0, 1, nx), lambda i, o: np.abs((i + o) % nx - i % nx) <= 1, 5)


def grid9(nx, ny, T, n=None):
    assert nx != ny
    n = nx * ny if n is None else n
    return _stencil(n, T, (-nx - 1, -nx, -nx + 1, -1, 0, 1, nx - 1, nx, nx + 1), lambda i, o: np.abs((i + o) % nx - i % nx) <= 1, 9)


def grid7(nx, ny, nz, T):
    """7-point stencil on an nx x ny x nz grid: +-1 absent at the ends of a grid row, +-nx at the ends of a plane"""
    n, pl = nx * ny * nz, nx * ny

    def neighbour(i, o):
        j = i + o
        return (np.abs(j % nx - i % nx) <= 1) & (np.abs((j % pl) // nx - (i % pl) // nx) <= 1)
    return _stencil(n, T, (-pl, -nx, -1, 0, 1, nx, pl), neighbour, 7)


def form_of(eu, A, T):
    """(pipeline_dia_diagonals, general_dia_diagonals, sell) of eu.host_pattern_info: the aliased narrow-band array, the general form's
    own array, and whether the SELL slots hold every entry (no overflow pass: the fused term kernels)"""
    pi = eu.host_pattern_info(A, T)
    return pi["pipeline_dia_diagonals"], pi["general_dia_diagonals"], bool(pi["sell"] and pi["sell_cut"] == 0)


def stored_ordering(eu, A, T):
    """None, or the ordering a default context stores A in at these sizes (capi.hip, maybe_reorder: reverse Cuthill-McKee is tried for an
    operator on the two-kernel step -- a complex type without a narrow band -- that is wider than the band the patch form takes in its
    own ordering, and kept when it reaches a better step form)"""
    perm, info = eu.host_rcm(A, T)
    ring_max = (16 // np.dtype(T).itemsize) * LIMITS["BLOCK"] // 8
    return perm if info["would_reorder"] and info["bandwidth_before"] > ring_max else None


# ---- the case table -------------------------------------------------------------------------------------------------------------
W8, D8, G32 = LIMITS["PIPE_WMAX"], LIMITS["PIPE_DIA_MAX"], LIMITS["GDIA_MAX"]
NARROW = {1: (-3,), 2: (-3, 0), 4: (-W8, -1, 0, 2), 6: (-W8, -3, 0, 1, 5, W8), 7: tuple(o for o in OFFS_HB8_D8 if o != 2), 8: OFFS_HB8_D8}
OFFS_13 = (-129, -40, -17, -9, -4, -1, 0, 1, 3, 8, 33, 100, 257)
# odd and even offsets, beyond a pack (1 .. 4 rows), a slice (64 .. 256 rows) and a 512-row unit of the array's leading dimension
_HALF = (1, 2, 3, 5, 7, 11, 13, 17, 64, 65, 130, 256, 257, 300)
OFFS_31 = tuple(sorted((0, 301, -299) + _HALF + tuple(-o for o in _HALF)))
OFFS_32 = tuple(sorted(OFFS_31 + (511,)))
OFFS_33 = tuple(sorted(OFFS_32 + (-511,)))
OFFS_ONE_SIDED = (1, 3, 64, 300)
N_WIDE = 700
assert len(OFFS_31) == G32 - 1 and len(set(OFFS_32)) == G32 and len(set(OFFS_33)) == G32 + 1 and len(OFFS_13) == 13
assert all(len(v) == k and max(abs(o) for o in v) <= W8 for k, v in NARROW.items()) and len(NARROW[8]) == D8


def wrap_offsets(n):
    return (-(n - 1), -1, 0, 1, n - 1)


def fill_drop(n, offsets, over, main_keep):
    """how many off-diagonal entries to remove so that nnz is the smallest that still meets analyze_pattern's zero-fill rule
    nd n <= 1.3 nnz + 1024 -- or (over) one entry fewer"""
    nd = len(offsets)
    full = sum(n - abs(o) for o in offsets) - int(round((1.0 - main_keep) * n))
    least = next(q for q in range(full, 0, -1) if not limits.fill_ok(nd, n, q - 1))
    assert limits.fill_ok(nd, n, least) and full > least
    return full - least + (1 if over else 0)


class Case:
    """name, the size and the operator per element type, alpha = |t| opnorm(A - mu I, Inf), and the form the analysis gives it:
    "aliased" (the narrow band's array), "general" (the general form's own array) or "sell" (no diagonal form), with nd diagonals"""

    def __init__(self, name, form, nd, make, alpha=40.0, tags=()):
        self.name, self.form, self.nd, self.make, self.alpha, self.tags = name, form, nd, make, alpha, frozenset(tags)

    def operator(self, T):
        return self.make(np.dtype(T))

    def expected(self):
        return {"aliased": (self.nd, 0, True), "general": (0, self.nd, True), "sell": (0, 0, True)}[self.form]

    def __repr__(self):
        return self.name


def _sizes(T):
    sh = slice_rows(T)
    return (("SH-1", sh - 1), ("SH", sh), ("SH+1", sh + 1), ("511", 511), ("512", 512), ("513", 513))


FILL_MAIN_KEEP = 0.5
CASES = [Case("band nd=%d" % k, "aliased", k, lambda T, o=o: diagonals(257, o, T), tags=("block",) if k == 7 else ()) for k, o in NARROW.items()]
CASES += [
    Case("nd=9", "general", 9, lambda T: diagonals(257, OFFS_HB8_D9, T), tags=("block", "grid", "phiv")),
    Case("nd=10", "general", 10, lambda T: diagonals(257, OFFS_HB8_D9 + (67,), T)),      # (two left over after two rounds of four)
    Case("nd=13", "general", 13, lambda T: diagonals(385, OFFS_13, T), tags=("block", "from_dia")),
    Case("nd=31", "general", 31, lambda T: diagonals(N_WIDE, OFFS_31, T)),
    Case("nd=32", "general", 32, lambda T: diagonals(N_WIDE, OFFS_32, T), tags=("block", "grid", "phiv", "inf")),
    Case("nd=33", "sell", 33, lambda T: diagonals(N_WIDE, OFFS_33, T), tags=("block",)),
    # explicit zeros up to the fill rule, half of the main diagonal among them: mu comes from a partly stored diagonal
    Case("nd=32 fill limit", "general", 32,
         lambda T: diagonals(N_WIDE, OFFS_32, T, drop=fill_drop(N_WIDE, OFFS_32, False, FILL_MAIN_KEEP), main_keep=FILL_MAIN_KEEP), tags=("inf", "mu")),
    Case("nd=32 fill limit + 1", "sell", 32,
         lambda T: diagonals(N_WIDE, OFFS_32, T, drop=fill_drop(N_WIDE, OFFS_32, True, FILL_MAIN_KEEP), main_keep=FILL_MAIN_KEEP)),
    # no stored diagonal entry at all (mu = 0), and rows without any entry at the end.  alpha: the truth is the weak side here -- against
    # the series summed in 80-bit arithmetic scipy's expm of this real triangular matrix (and of its augmented form with p = 8) is
    # 5 .. 15 eps off at alpha = 14 .. 16, 50 .. 180 eps at alpha = 12 and 20 .. 100 eps at alpha = 20, while the restatement stays
    # within 3 eps of that series at all of them
    Case("one-sided", "general", 4, lambda T: diagonals(385, OFFS_ONE_SIDED, T), alpha=15.0, tags=("phiv", "mu")),
    # the guard at +-(n - 1): one entry in the first row's last column and one in the last row's first
    Case("wrap", "general", 5, lambda T: diagonals(257, wrap_offsets(257), T), alpha=20.0, tags=("mu",)),
    Case("grid5 29x23", "general", 5, lambda T: grid5(29, 23, T), tags=("block", "grid", "phiv")),
    Case("grid9 19x31", "general", 9, lambda T: grid9(19, 31, T)),
    Case("grid7 7x8x11", "general", 7, lambda T: grid7(7, 8, 11, T)),
]
for _i in range(6):      # n on either side of a slice of the element type and of the 512-row unit of the diagonal array
    CASES.append(Case("nd=9 n=%s" % _sizes(np.float64)[_i][0], "general", 9, lambda T, i=_i: diagonals(_sizes(T)[i][1], OFFS_HB8_D9, T)))
    CASES.append(Case("grid5 n=%s" % _sizes(np.float64)[_i][0], "general", 5, lambda T, i=_i: grid5(19, 28, T, n=_sizes(T)[i][1])))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


PHIV_PS = (1, 8)      # B = [u_0 ... u_p] of the phiv_taylor cases


def tagged(tag):
    return [c for c in CASES if tag in c.tags]


# the smallest 2-D stencil that a default context stores in the grid-patch ordering: capi.hip detect_grid2d wants rows of k >= 64 cells
# and n >= 8 k; 15 grid rows make two tiles for the 8-byte types and four for ComplexF64
PATCH_GRID = (64, 15)
