"""Inputs with an exactly known exponential for the balanced dense device exponential (expv_mi_expm_balanced, expv_mi_gebal;
csrc/dense_dev.hip), and the CPU side of their checks; no device work here.

* scaled(T, n, E, seed): A = D B D^-1 with B randn scaled to |B|_1 = 2 (rounded to T) and D = diag(2^e_i), e_i uniform integers in
  [-E, E].  D is a power-of-two scaling, so A is exact in T and exp(A) = D exp(B) D^-1 is exact given scipy's complex128 exp(B).
* isolated(T, n, a, c, E, seed): a random symmetric permutation of D C D^-1, C = [[T1 X Y], [0 M Z], [0 0 T2]] with T1 (a x a) and T2
  (c x c) upper triangular, |C|_1 = 2, and D = diag(I, 2^e, I): the middle block is badly scaled (and with it X and Z), the rows of
  T2 and the columns of T1 are what xGEBAL's permutation phase isolates.  The truth is again D exp(C) D^-1, permuted.
* degenerate(name, T): a permuted triangular matrix (the l == 1 return), a diagonal one, all zeros, a zero row and column inside a
  full matrix (with job 'B' the permutation phase isolates that index: the scaling loop's c == 0 || r == 0 skip cannot be reached
  once rows and columns without off-diagonal entries are gone), n = 1, and off-diagonal entries equal to -0.0 that must count as zero.
* gebal_restated(A): host_dense.h's gebal restated in numpy the way the DEVICE evaluates it -- the decisions and their order are
  the host's, every norm is evaluated in fp64 whatever the element type, the guards sfmin / sfmax are those of the element type --
  recording the smallest relative margin of the comparisons c < g, g >= r, (c + r) >= 0.95 s.  A case counts only with a margin of
  at least MARGIN = 1e-9, far above any fp64 summation-order difference at these n (n eps = 2.4e-13 at n = 1100); a seed that
  misses is replaced by the next one (seed + 1000), never skipped."""
import functools

import numpy as np
import scipy.linalg as sl

from tests import dense_cases as dc

MARGIN = 1e-9
BAL_MAX_SWEEPS = 128            # csrc/dense_dev.hip
TYPES = ("float64", "complex128", "float32", "complex64")


def _wide(T):
    return np.complex128 if np.dtype(T).kind == "c" else np.float64


def guards(T):
    """sfmin1, sfmax1, sfmin2, sfmax2 of xGEBAL for the real type of T (as doubles)"""
    fi = np.finfo(dc.real_type(T))
    sfmin1 = float(fi.tiny) / float(fi.eps)
    sfmax1 = 1.0 / sfmin1
    sfmin2 = sfmin1 * 2.0
    return sfmin1, sfmax1, sfmin2, 1.0 / sfmin2


def _nrm2(v, f32=False):
    """sqrt(sum |v|^2) in fp64: the plain sum where it stays inside (1e-280, 1e280), the scaled form otherwise.
    f32: squares and sum in float32 instead (a deliberately wrong variant: gebal_restated's mutate="float32_sums")"""
    if f32:
        re, im = np.real(v).astype(np.float32), np.imag(v).astype(np.float32)
        return float(np.sqrt(np.sum(re * re + im * im, dtype=np.float32)))
    re, im = np.real(v).astype(np.float64), np.imag(v).astype(np.float64)
    ss = float(np.sum(re * re + im * im))
    if 1e-280 < ss < 1e280:
        return float(np.sqrt(ss))
    amax = float(max(np.max(np.abs(re), initial=0.0), np.max(np.abs(im), initial=0.0)))
    if not amax > 0.0:
        return 0.0
    return amax * float(np.sqrt(np.sum((re / amax) ** 2 + (im / amax) ** 2)))


def _rel_margin(x, y):
    m = max(abs(x), abs(y))
    return abs(x - y) / m if m > 0 else np.inf


def gebal_restated(A, mutate=None):
    """xGEBAL job 'B' of A (not modified).  Returns a dict: ilo, ihi (1-based), scale (float64, LAPACK's convention), A_bal (in A's
    type), pos (position -> original index, 0-based), sweeps, margin, norm1 (fp64 1-norm of A_bal), order, s.
    mutate: None, or "no_diagonal" / "columns_from_one" / "float32_sums" -- deliberately wrong variants for tests of the tests."""
    A = np.asarray(A)
    T = A.dtype
    n = A.shape[0]
    out = {"margin": np.inf, "sweeps": 0}
    scale = np.ones(n)
    if n == 0:
        out.update(ilo=1, ihi=0, scale=scale, A_bal=A.copy(), pos=np.zeros(0, dtype=np.int64), norm1=0.0, order=3, s=0)
        return out
    NZ = (np.real(A) != 0) | (np.imag(A) != 0)          # -0.0 is zero
    np.fill_diagonal(NZ, False)
    pos = np.arange(n)
    k, l = 1, n
    early = False

    def swap(j, m):
        scale[m - 1] = j
        pos[[j - 1, m - 1]] = pos[[m - 1, j - 1]]

    noconv = True
    while noconv and not early:
        noconv = False
        for i in range(l, 0, -1):
            if not NZ[pos[i - 1], pos[:l]].any():
                swap(i, l)
                noconv = True
                if l == 1:
                    early = True
                    break
                l -= 1
    if early:
        k = l = 1
    else:
        noconv = True
        while noconv:
            noconv = False
            for j in range(1 if mutate == "columns_from_one" else k, l + 1):
                if k > l:      # (only the mutated scan can get here)
                    break
                if not NZ[pos[k - 1:l], pos[j - 1]].any():
                    swap(j, k)
                    noconv = True
                    k += 1
        scale[k - 1:l] = 1.0
    W = np.array(A[np.ix_(pos, pos)], dtype=_wide(T), order="F")      # P'AP, scaled eagerly below: exact, the factors are powers of two
    if not early:
        sfmin1, sfmax1, sfmin2, sfmax2 = guards(T)
        cab = lambda z: np.abs(np.real(z)) + np.abs(np.imag(z))
        margin = np.inf
        noconv = True
        while noconv and out["sweeps"] < BAL_MAX_SWEEPS:
            noconv = False
            for i in range(k, l + 1):
                colv, rowv = W[k - 1:l, i - 1], W[i - 1, k - 1:l]
                if mutate == "no_diagonal":
                    colv, rowv = np.delete(colv, i - k), np.delete(rowv, i - k)
                c, r = _nrm2(colv, mutate == "float32_sums"), _nrm2(rowv, mutate == "float32_sums")
                ica = int(np.argmax(cab(W[:l, i - 1])))
                ca = float(abs(W[ica, i - 1]))
                ira = int(np.argmax(cab(W[i - 1, k - 1:])))
                ra = float(abs(W[i - 1, ira + k - 1]))
                if c == 0.0 or r == 0.0:
                    continue
                g, f, s = r / 2.0, 1.0, c + r
                while True:
                    margin = min(margin, _rel_margin(c, g))
                    if not (c < g and max(f, c, ca) < sfmax2 and min(r, g, ra) > sfmin2):
                        break
                    f *= 2.0; c *= 2.0; ca *= 2.0; r /= 2.0; g /= 2.0; ra /= 2.0
                g = c / 2.0
                while True:
                    margin = min(margin, _rel_margin(g, r))
                    if not (g >= r and max(r, ra) < sfmax2 and min(f, c, g, ca) > sfmin2):
                        break
                    f /= 2.0; c /= 2.0; g /= 2.0; ca /= 2.0; r *= 2.0; ra *= 2.0
                margin = min(margin, _rel_margin(c + r, 0.95 * s))
                if (c + r) >= 0.95 * s:
                    continue
                if f < 1.0 and scale[i - 1] < 1.0 and f * scale[i - 1] <= sfmin1:
                    continue
                if f > 1.0 and scale[i - 1] > 1.0 and scale[i - 1] >= sfmax1 / f:
                    continue
                scale[i - 1] *= f
                noconv = True
                W[i - 1, k - 1:] *= 1.0 / f
                W[:l, i - 1] *= f
            out["sweeps"] += 1
        out["margin"] = margin
    with np.errstate(over="ignore"):
        A_bal = np.asfortranarray(W.astype(T))
    nb = dc.norm1_f64(A_bal)
    order, s = dc.expected_method(nb)
    out.update(ilo=k, ihi=l, scale=scale, A_bal=A_bal, pos=pos.copy(), norm1=nb, order=order, s=s)
    return out


def unbalance(X, ilo, ihi, scale):
    """host_dense.h's unbalance on a copy of X (any type): the scaling undone, the lower exchanges in reverse, the upper ones forward"""
    X = np.array(X, order="F", copy=True)
    n = X.shape[0]
    for j in range(ilo, ihi + 1):
        X[j - 1, :] *= scale[j - 1]
        X[:, j - 1] /= scale[j - 1]
    order = list(range(ilo - 1, 0, -1)) + list(range(ihi + 1, n + 1))
    for j in order:
        m = int(scale[j - 1])
        if m != j:
            X[[j - 1, m - 1], :] = X[[m - 1, j - 1], :]
            X[:, [j - 1, m - 1]] = X[:, [m - 1, j - 1]]
    return X


def balanced_restatement(A):
    """exponential!(A, ExpMethodHigham2005Base()) in A's own type: gebal_restated, dense_cases.restatement, unbalance.
    Returns (exp(A), the gebal dict)."""
    g = gebal_restated(A)
    X, _, order, s = dc.restatement(g["A_bal"])
    assert (order, s) == (g["order"], g["s"])
    R = dc.real_type(A.dtype).type
    return unbalance(X, g["ilo"], g["ihi"], g["scale"].astype(R)), g


# ------------------------------------------------------------------------------------------- families
@functools.lru_cache(maxsize=None)
def _base(tname, n, seed, norm1=2.0):
    """(B in the element type with |B|_1 = norm1 before rounding, exp(B) in complex128)"""
    T = np.dtype(tname)
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    if T.kind == "c":
        B = B + 1j * rng.standard_normal((n, n))
    B = (B * (norm1 / np.linalg.norm(B, 1))).astype(T)
    return B, sl.expm(B.astype(np.complex128))


def _finish(A, truth, **extra):
    A = np.asfortranarray(A)
    A.setflags(write=False)
    g = gebal_restated(A)
    return dict(A=A, truth=truth, gebal=g, **extra)


def _scaled_once(tname, n, E, seed):
    T = np.dtype(tname)
    B, eB = _base(tname, n, seed)
    e = np.random.default_rng(seed + 77).integers(-E, E + 1, size=n)
    D = np.ldexp(1.0, e)
    A = (B.astype(_wide(T)) * D[:, None] / D[None, :]).astype(T)
    assert np.array_equal(A.astype(_wide(T)) * D[None, :] / D[:, None], B.astype(_wide(T)))      # exact in T
    return _finish(A, eB * D[:, None] / D[None, :], D=D, seed=seed)


def _with_margin(build, seed, margin):
    for t in range(50):
        c = build(seed + 1000 * t)
        if c["gebal"]["margin"] >= margin:
            return c
    raise AssertionError("no seed with the required margin")


@functools.lru_cache(maxsize=None)
def scaled(tname, n, E, seed=None, margin=MARGIN):
    """dict: A (read-only, column-major, type T), truth (complex128), D, gebal (gebal_restated(A)), seed (the one that was taken)"""
    seed = 100 * n + E if seed is None else seed
    return _with_margin(lambda sd: _scaled_once(tname, n, E, sd), seed, margin)


def clip_blocks(n, a, c):
    """the triangular block sizes that fit n and leave a middle block of at least 2 (n >= 2)"""
    while a + c > max(n - 2, 0):
        if a >= c and a > 0:
            a -= 1
        elif c > 0:
            c -= 1
    return a, c


def _isolated_once(tname, n, a, c, E, seed):
    T = np.dtype(tname)
    a, c = clip_blocks(n, a, c)
    rng = np.random.default_rng(seed)
    Cm = rng.standard_normal((n, n))
    if T.kind == "c":
        Cm = Cm + 1j * rng.standard_normal((n, n))
    m = n - a - c
    Cm[a:, :a] = 0
    Cm[a + m:, a:a + m] = 0
    Cm[:a, :a] = np.triu(Cm[:a, :a])
    Cm[a + m:, a + m:] = np.triu(Cm[a + m:, a + m:])
    Cm = (Cm * (2.0 / np.linalg.norm(Cm, 1))).astype(T)
    e = np.zeros(n, dtype=np.int64)
    e[a:a + m] = rng.integers(-E, E + 1, size=m)
    D = np.ldexp(1.0, e)
    A = (Cm.astype(_wide(T)) * D[:, None] / D[None, :]).astype(T)
    truth = sl.expm(Cm.astype(np.complex128)) * D[:, None] / D[None, :]
    p = rng.permutation(n)
    return _finish(A[np.ix_(p, p)], truth[np.ix_(p, p)], blocks=(a, m, c), seed=seed)


@functools.lru_cache(maxsize=None)
def isolated(tname, n, a, c, E=12, seed=None, margin=MARGIN):
    seed = 100 * n + 10 * a + c if seed is None else seed
    return _with_margin(lambda sd: _isolated_once(tname, n, a, c, E, sd), seed, margin)


DEGENERATE = ("permuted_triangular", "diagonal", "zero", "zero_row_and_column", "one", "negative_zeros")


@functools.lru_cache(maxsize=None)
def degenerate(name, tname):
    T = np.dtype(tname)
    rng = np.random.default_rng(len(name))
    cx = (lambda s: 1j * rng.standard_normal(s)) if T.kind == "c" else (lambda s: 0)
    if name == "permuted_triangular":
        n = 9
        M = np.triu(rng.standard_normal((n, n)) + cx((n, n))) * np.ldexp(1.0, rng.integers(-6, 7, size=(n, n)))
        p = rng.permutation(n)
        M = M[np.ix_(p, p)]
    elif name == "diagonal":
        M = np.diag(rng.standard_normal(6) + cx(6))
    elif name == "zero":
        M = np.zeros((5, 5))
    elif name == "zero_row_and_column":
        n = 12
        M = (rng.standard_normal((n, n)) + cx((n, n))) * np.ldexp(1.0, rng.integers(-8, 9, size=n))[:, None]
        M[4, :] = 0
        M[:, 4] = 0
    elif name == "one":
        M = np.array([[0.75]]) + cx((1, 1))
    else:      # an upper Hessenberg-like full block whose strictly lower part is -0.0: isolated only if -0.0 counts as zero
        n = 8
        M = np.triu(rng.standard_normal((n, n)) + cx((n, n)))
        M[np.tril_indices(n, -1)] = -0.0
        p = rng.permutation(n)
        M = M[np.ix_(p, p)]
    M = M * (1.5 / max(np.linalg.norm(M, 1), 1e-300)) if np.any(M != 0) else M
    A = np.asfortranarray(M.astype(T))
    if name == "negative_zeros":
        assert np.count_nonzero(np.signbit(np.real(A)) & (A == 0)) >= 20
    truth = sl.expm(A.astype(np.complex128))
    return _finish(A, truth)


def same_bits(X, Y):
    """equal as numbers AND in the sign of every zero"""
    X, Y = np.asarray(X), np.asarray(Y)
    return (X.dtype == Y.dtype and X.shape == Y.shape and np.array_equal(X, Y)
            and np.array_equal(np.signbit(np.real(X)), np.signbit(np.real(Y))) and np.array_equal(np.signbit(np.imag(X)), np.signbit(np.imag(Y))))


def recovered_D(case):
    """log2 of scale / D along the positions of a `scaled` case: constant when balancing recovers D up to a common factor"""
    g = case["gebal"]
    return np.log2(g["scale"]) - np.log2(case["D"][g["pos"]])


@functools.lru_cache(maxsize=None)
def unbalanced_cpu_error(tname, n, E):
    """error of Higham 2005 WITHOUT balancing (dense_cases.restatement, the element type's arithmetic on the CPU) on scaled(T, n, E):
    what the device's expv_mi_expm is predicted to do on that matrix (NaN where the squarings overflow)"""
    case = scaled(tname, n, E)
    with np.errstate(all="ignore"):
        return dc.rel_err(dc.restatement(case["A"])[0], case["truth"])


@functools.lru_cache(maxsize=None)
def float32_sums_case(tname):
    """A 3 x 3 matrix of a 32-bit type whose first decision needs the fp64 sums: column 1 has norm 1, row 1 has the entries 8 and
    2^-10, so r^2 = 64 + 2^-20 -- in float32 the small square is an eighth of an ulp of 64 and vanishes in ANY order of summation.
    With r = 8 (1 + 2^-27) the second doubling (2 < r / 4) is taken, by a relative margin of 2^-27 = 7.5e-9 >= MARGIN, and d_1
    becomes 4; with r = 8 it is not, and d_1 becomes 2.  dict as the other families' (truth: scipy's, the matrix is tame)."""
    T = np.dtype(tname)
    assert dc.real_type(T) == np.float32
    u = 1j if T.kind == "c" else 1.0
    A = np.array([[0, 8 * u, 2.0 ** -10], [u, 0, 0], [0, 1, 0]], dtype=T)
    return _finish(A, sl.expm(A.astype(np.complex128)))
