"""exp(r_k t A) b on a time grid by one sweep of the truncated Taylor series (expv_mi_expv_taylor_grid) restated in numpy, the
grids its tests run on, and the truth they are held to.

restated_grid() follows expv_taylor_cases.restated() line by line for F and v (so its column at r = R is that function's result,
bit for bit) and adds the outputs as include/expv_mi.h defines them: classification in double, G_k = F + sum_j d_kj v_j with
d_kj = d_k,j-1 rho_k in double rounded to the real type, the stopping test c1 + c2 <= tol |G_k|_inf with c2 = d_kj |v_j|_inf, masking,
the closing factor exp(mu rho_k h).  The tests of the outputs are evaluated in the real type, as restated() evaluates F's.

Truth.  Per output it is scipy.linalg.expm(r_k t A) b.  For n <= 257 that is what truth_columns() computes, one expm per distinct
r_k.  At n = 1000 one expm costs 0.5 .. 1 s, and the grids hold 40 .. 110 outputs for each of 20 operator / type pairs: some ten
minutes of expm where a test may take seconds.  There the grids lie on a lattice r_k = k / L and the truth is expm(t A / L)^k b: ONE
expm of a matrix of norm about 1 (no squaring phase) and L products with a vector.  Both are roundings of the same vector; how far
apart may they be?  For the symmetric tridiagonal case (n = 1000, alpha = 40) the direct expm, the product form and an
eigendecomposition disagree pairwise by 8 .. 110 eps at the outputs, the two expm routes by 21 eps at r = 1, where the product form is
40 steps deep: the vector has decayed, and every route carries errors relative to |b|, not to the result.  That is the reference's own
error at this size.  lattice_truth() measures three of its columns -- a quarter of the way, half way and the last -- against the
direct expm((k / L) t A) b for every case; beyond LATTICE_GAP = 64 eps, half the cap the restatement is held to against this
reference, it does not serve as truth and grid_truth() computes one direct expm per output instead (dense ComplexF64 on the lattice
of the 2^-24 table, L = 60: 70.5 eps).  The largest of the three gaps goes to the parity table."""
import math

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

from tests import expv_taylor_cases as tc


# ---- the classification ------------------------------------------------------------------------------------------------------
def classify(s, r):
    """(stage, rho, kind) with exactly the expressions of the header: x = s (r / R), i = max(ceil(x) - 1, 0), rho = x - i"""
    r = np.asarray(r, dtype=np.float64)
    R = float(r.max()) if r.size else 0.0
    stage, rho, kind = np.full(r.size, -1, dtype=np.int64), np.zeros(r.size), np.zeros(r.size, dtype=np.int32)
    for k in range(r.size):
        if r[k] == 0.0:
            continue
        x = float(s) * (float(r[k]) / R)
        i = max(math.ceil(x) - 1.0, 0.0)
        stage[k], rho[k] = int(i), x - i
        kind[k] = 2 if rho[k] == 1.0 else 1
    return stage, rho, kind


def interior_counts(s, r):
    """interior outputs per stage 0 .. s-1"""
    stage, _, kind = classify(s, r)
    return [int(np.sum((stage == i) & (kind == 1))) for i in range(s)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def restated_grid(t, r, A, b, T, alpha, theta, tol, mu=None):
    """Column k = exp(r_k t A) b in element type T; alpha = |R t| opnorm(A - mu I, Inf).  Returns (W, info): info has m, s,
    applications (terms computed, shared by all outputs), early_stages, nonfinite_stage and the per-output lists stage, terms, kind."""
    T = np.dtype(T)
    Rt = np.finfo(T).dtype.type
    r = np.asarray(r, dtype=np.float64)
    n, q = A.shape[0], r.size
    R = float(r.max()) if q else 0.0
    Tt = R * t
    A = sp.csr_matrix(A).astype(T) if sp.issparse(A) else np.asarray(A, dtype=T)
    if mu is None:
        mu = tc.shift_norm(A, Tt)[0]
    m, s = tc.params(alpha, theta)
    stage, rho, kind = classify(s, r)
    cplx = T.kind == "c"
    muT, tolR = T.type(mu), Rt(tol)

    def factor(z):      # exp(z) as the element type holds it
        return T.type(np.exp(complex(z))) if cplx else T.type(math.exp(float(np.real(z))))
    eta = factor(complex(mu) * complex(Tt) / s)
    h = complex(Tt) / s
    F = np.array(b, dtype=T)
    v = F.copy()
    W = np.zeros((n, q), dtype=T)
    terms = [0] * q
    for k in range(q):
        if kind[k] == 0:
            W[:, k] = F
    info = {"m": m, "s": s, "applications": 0, "early_stages": 0, "nonfinite_stage": 0}
    with np.errstate(all="ignore"):
        for st in range(s):
            inner = [k for k in range(q) if stage[k] == st and kind[k] == 1]
            ends = [k for k in range(q) if stage[k] == st and kind[k] == 2]
            c1 = np.max(np.abs(v)) if n else Rt(0)
            G = {k: F.copy() for k in inner}
            if m == 0:      # alpha = 0: exp(mu r_k t) b
                for k in inner:
                    z = factor(complex(mu) * (float(r[k]) * complex(t)))
                    G[k] = (F * z).astype(T) if z != 1 else F.copy()
            elif c1 == 0:
                info["early_stages"] += 1      # a zero vector stays zero: nothing is applied, every output of the stage is F
            else:
                d = {k: 1.0 for k in inner}
                c1g = {k: c1 for k in inner}
                live, flive, fterms = set(inner), True, 0
                for j in range(1, m + 1):
                    if not flive and not live:
                        break
                    c = T.type(complex(Tt) / s / j) if cplx else T.type(float(np.real(Tt)) / s / j)
                    v = ((A @ v - muT * v) * c).astype(T)
                    info["applications"] += 1
                    c2 = np.max(np.abs(v))
                    if flive:
                        F = (F + v).astype(T)
                        fterms += 1
                        nF = np.max(np.abs(F))
                        if Rt(c1 + c2) <= Rt(tolR * nF):
                            info["early_stages"] += int(j < m)
                            flive = False
                        else:
                            c1 = c2
                    for k in sorted(live):
                        d[k] = d[k] * float(rho[k])
                        dk = Rt(d[k])
                        G[k] = (G[k] + dk * v).astype(T)
                        terms[k] += 1
                        c2k = Rt(dk * c2)
                        if Rt(c1g[k] + c2k) <= Rt(tolR * np.max(np.abs(G[k]))):
                            live.discard(k)
                        else:
                            c1g[k] = c2k
                for k in inner:
                    z = factor(complex(mu) * (float(rho[k]) * h))
                    if z != 1:
                        G[k] = (G[k] * z).astype(T)
                for k in ends:
                    terms[k] = fterms
            for k in inner:
                W[:, k] = G[k]
            if eta != 1:
                F = (F * eta).astype(T)
            v = F.copy()
            for k in ends:
                W[:, k] = F
            if not np.all(np.isfinite(v)):
                info["nonfinite_stage"] = st + 1
                for k in range(q):
                    if stage[k] > st:
                        W[:, k] = F      # every output of a later stage is the non-finite F as it stands
                break
    info.update(stage=[int(x) for x in stage], terms=terms, kind=[int(x) for x in kind])
    return W, info


# ---- the grids ---------------------------------------------------------------------------------------------------------------
def rand13():
    """11 seeded uniform fractions (one of them twice) with 1.0 and 0.0 among them, unsorted"""
    u = tc.rng_of(13, 77).random(11)
    u[7] = u[2]
    return np.concatenate([u[:4], [1.0], u[4:9], [0.0], u[9:]])


def lin40():
    return np.linspace(0.025, 1.0, 40)


PANEL_COUNTS = (0, 1, 2, 3, 5, 8, 9, 17)
PANEL_SLOTS = 20      # the interior outputs of a stage lie at j / 20 of it, j = 1 .. 19


def panel_grids(s):
    """Grids (with the per-stage interior counts they were built for) on the lattice k / (20 s) that together give the stages the
    counts 0, 1, 2, 3, 5, 8, 9 and 17; every grid ends with 1.0.  The caller checks the counts with host_taylor_grid_plan."""
    out = []
    for g0 in range(0, len(PANEL_COUNTS), s):
        counts = list(PANEL_COUNTS[g0:g0 + s]) + [0] * max(0, s - len(PANEL_COUNTS[g0:]))
        ks = []
        for i, c in enumerate(counts):
            slots = [1 + (j * (PANEL_SLOTS - 1)) // max(c, 1) for j in range(c)]      # c distinct slots in 1 .. 19
            ks += [i * PANEL_SLOTS + j for j in slots]
        ks.append(s * PANEL_SLOTS)
        r = np.array(ks, dtype=np.float64) / float(s * PANEL_SLOTS)
        out.append((r, counts))
    return out


# ---- truth -------------------------------------------------------------------------------------------------------------------
def as_dense(A, W):
    return (A.toarray() if sp.issparse(A) else np.asarray(A)).astype(W)


def truth_columns(A, b, t, r):
    """expm(r_k t A) b per output, one expm per distinct r_k (n <= 257)"""
    W = tc.wide(A.dtype)
    Ad, bw = as_dense(A, W), np.asarray(b).astype(W)
    cols = {}
    for x in r:
        if float(x) not in cols:
            cols[float(x)] = sl.expm((float(x) * t) * Ad) @ bw
    return np.stack([cols[float(x)] for x in r], axis=1)


LATTICE_GAP = 64.0


def lattice_truth(A, b, t, L):
    """columns k = 0 .. L of expm(t A / L)^k b = expm((k / L) t A) b, and how far the columns L / 4, L / 2 and L are from the direct
    expm((k / L) t A) b (the largest of the three)"""
    W = tc.wide(A.dtype)
    Ad, bw = as_dense(A, W), np.asarray(b).astype(W)
    E = sl.expm((t / L) * Ad)
    cols = [bw]
    for _ in range(L):
        cols.append(E @ cols[-1])
    X = np.stack(cols, axis=1)
    gap = max(tc.relmax(X[:, k], sl.expm(((k / float(L)) * t) * Ad) @ bw) for k in sorted({max(L // 4, 1), max(L // 2, 1), L}))
    return X, gap


def grid_truth(A, b, t, r, L, lattice):
    """The truth of the grid r on the lattice k / L: the lattice's columns where its gap is within LATTICE_GAP, else -- the product
    form is no truth for this case -- one direct expm per distinct output, as for the small sizes.  lattice = lattice_truth(A, b, t, L)."""
    X, gap = lattice
    if gap <= LATTICE_GAP * tc.eps_of(tc.wide(A.dtype)):
        return X[:, lattice_index(r, L)]
    return truth_columns(A, b, t, r)


def lattice_index(r, L):
    """the lattice point k of every r_k = k / L (the grids of this file are built that way)"""
    k = np.rint(np.asarray(r) * L).astype(np.int64)
    assert np.all(np.abs(k / float(L) - np.asarray(r)) <= 2.0 ** -52 * np.asarray(r)), "a grid off its lattice"
    return k


def relmax_columns(Wd, Wt):
    """relative max-norm error per column"""
    return [tc.relmax(Wd[:, k], Wt[:, k]) for k in range(Wt.shape[1])]
