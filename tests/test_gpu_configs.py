"""GPU parity tests of the BASELINE configurations that round 1 left untested or unchecked at size:

    C3  phiv_timestep adaptive, K = 4, DENSE fp64 A          (/root/reference/test/basictests.jl:666-691 pattern)
        + the same through _phiv_timestep_caches             (krylov_phiv_adaptive.jl:320-324, :502-511; basictests.jl:576-648)
    C4  kiops, complex sparse, iop = 2 at n = 1e6            (no reference method: extension; vs the oracle's same extension,
                                                              the group property and the dense truth at small n)
    C5  batch of independent expv at n = 1e5                 (vs the plain-C oracle per column)

and of the defects the round-1 advisor found by reading: a context-cached kiops workspace must behave like the
reference's fresh KrylovSubspace; a host matrix mutated in place between calls must be read again; malformed CSR/CSC input
returns ArgumentError instead of crashing; a device-resident dense Hermitian matrix takes the Lanczos path by default.

Every comparison prints the measured error next to its bar (tests/_util.close)."""
import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from oracle import c_oracle as co
from oracle import krylov_oracle as ko
from tests._util import c2_operator, close, dense_phis, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


def c3_inputs(n, K=4):
    """A = -2I + randn/sqrt(n) (seed 4), B = randn(n, K+1) (seed 5)."""
    A = -2.0 * np.eye(n) + np.random.default_rng(4).standard_normal((n, n)) / np.sqrt(n)
    B = np.asfortranarray(np.random.default_rng(5).standard_normal((n, K + 1)))
    return A, B


# ------------------------------------------------------------------ C3 ------------------------------------------------
@pytest.mark.parametrize("n,ts,tol", [(1500, [1.0], 1e-7), (1500, [6.0], 1e-7), (1500, [3.0, 12.0, 7.5], 1e-9),
                                      (257, [2.5, 5.0], 1e-7)])
def test_c3_dense_adaptive_phiv_timestep_matches_oracle(eu, n, ts, tol):
    """BASELINE configs[2] workload at sizes the numpy oracle finishes in seconds (the literal t = 1 case is one accepted
    sub-step; the longer horizons make the controller reject, grow m and cut tau): same controller decisions (sub-steps,
    operator applications, final m) and the same snapshots."""
    A, B = c3_inputs(n)
    st, so = {}, {}
    U = eu.phiv_timestep(np.array(ts), A, B, adaptive=True, tol=tol, stats=st)
    Uo = ko.phiv_timestep(np.array(ts), A, B, adaptive=True, tol=tol, stats=so)
    assert (st["num_timesteps"], st["matvecs"], st["m"]) == (so["num_timesteps"], so["matvecs"], so["m"]), (st, so)
    close(U, Uo, 1e-12, "C3 dense adaptive phiv_timestep U vs oracle (n=%d, ts=%s, tol=%g)" % (n, ts, tol))


def test_c3_dense_adaptive_vs_dense_truth(eu):
    """basictests.jl:666-691 with a dense non-symmetric operator: snapshots against the block-matrix phi functions."""
    n, K, t, tol = 120, 4, 3.0, 1e-7
    A, B = c3_inputs(n, K)
    Ph, Phh = dense_phis(t * A, K), dense_phis(t / 2 * A, K)
    u_exact = sum(t ** i * Ph[i] @ B[:, i] for i in range(K + 1))
    uhalf = sum((t / 2) ** i * Phh[i] @ B[:, i] for i in range(K + 1))
    U = eu.phiv_timestep(np.array([t / 2, t]), A, B, adaptive=True, tol=tol)
    close(U[:, 0], uhalf, tol, "C3-style dense adaptive, t/2 vs dense truth")
    close(U[:, 1], u_exact, tol, "C3-style dense adaptive, t vs dense truth")
    u0 = eu.expv_timestep(t, A, B[:, 0], adaptive=True, tol=tol)          # p = 0 special case
    close(u0, Ph[0] @ B[:, 0], tol, "C3-style dense adaptive expv_timestep vs dense truth")


def test_c3_timestep_caches_reuse_and_growth(eu):
    """_phiv_timestep_caches (krylov_phiv_adaptive.jl:502-511): the caches tuple (u, W, P, Ks, phiv_cache) is reused over
    calls, W / P may be wider than needed (:321-324), an undersized subspace grows (resize!, arnoldi.jl:355-357), a cache
    of the wrong length trips the @assert (:320)."""
    n, K = 600, 4
    A, B = c3_inputs(n, K)
    op = eu.MIOperator(A)
    caches = eu.timestep_caches(B[:, 0], 30, K)            # maxiter 30, p = 4
    ref = ko.phiv_timestep(np.array([0.5, 1.0]), A, B, adaptive=True, tol=1e-7)
    for rep in range(3):                                   # the same caches, call after call
        st = {}
        U = np.empty((n, 2), order="F")
        eu.phiv_timestep_(U, np.array([0.5, 1.0]), op, B, adaptive=True, tol=1e-7, caches=caches, stats=st)
        close(U, ref, 1e-12, "C3 through timestep_caches, call %d" % rep)
    # fewer coefficient columns than the caches were made for: views of W / P
    U1 = np.empty((n, 1), order="F")
    eu.phiv_timestep_(U1, np.array([1.0]), op, B[:, :3], adaptive=True, tol=1e-7, caches=caches)
    close(U1, ko.phiv_timestep(np.array([1.0]), A, B[:, :3], adaptive=True, tol=1e-7), 1e-12, "caches wider than needed")
    # subspace smaller than the m the controller asks for: grows inside arnoldi!
    small = eu.timestep_caches(B[:, 0], 4, K)
    U2 = np.empty((n, 2), order="F")
    eu.phiv_timestep_(U2, np.array([0.5, 1.0]), op, B, adaptive=True, tol=1e-7, caches=small)
    close(U2, ref, 1e-12, "undersized cache grows")
    # non-adaptive with the caches and a different right-hand side afterwards (state of the previous call must not leak)
    B2 = np.asfortranarray(np.random.default_rng(99).standard_normal((n, K + 1)))
    U3 = np.empty((n, 1), order="F")
    eu.phiv_timestep_(U3, np.array([0.3]), op, B2, m=20, tol=1e-9, caches=caches)
    close(U3, ko.phiv_timestep(np.array([0.3]), A, B2, m=20, tol=1e-9), 1e-12, "caches reused with other inputs")
    with pytest.raises(AssertionError):
        eu.phiv_timestep_(U3, np.array([0.3]), op, B2, caches=eu.timestep_caches(np.empty(n + 1), 10, K))
    with pytest.raises(AssertionError):                    # more coefficient columns than W / P hold
        eu.phiv_timestep_(U3, np.array([0.3]), op, B2, caches=eu.timestep_caches(B[:, 0], 10, 2))


def test_c3_device_resident_dense_operator(eu):
    """The C3 bench hands over A as a device tensor (214 GB cannot be staged): ishermitian / opnorm / nnz come from the
    device pass at create time and the result equals the host-matrix path."""
    import torch
    n = 700
    A, B = c3_inputs(n)
    Ad = torch.as_tensor(np.asfortranarray(A).T.copy(), device="cuda").t()      # column-major device matrix
    opd, oph = eu.MIOperator(Ad), eu.MIOperator(A)
    assert opd.ishermitian == oph.ishermitian == False
    assert opd.nnz == oph.nnz == n * n
    close(opd.opnorm_inf, oph.opnorm_inf, 1e-14, "device opnorm(A, Inf)")
    U = eu.phiv_timestep(np.array([1.0]), opd, B, adaptive=True, tol=1e-7)
    close(U, eu.phiv_timestep(np.array([1.0]), oph, B, adaptive=True, tol=1e-7), 1e-13, "device-resident vs host dense operator")
    S = (A + A.T) / 2
    S[3, 5] = S[5, 3] = 0.0
    Sd = torch.as_tensor(S, device="cuda")
    ops = eu.MIOperator(Sd)
    assert ops.ishermitian and ops.nnz == n * n - 2
    b = np.random.default_rng(1).standard_normal(n)
    Ks = eu.arnoldi(ops, b, m=20)                        # default: ishermitian(A) -> lanczos!, U real
    Ko = ko.arnoldi(S, b, m=20)
    assert Ks.U == np.float64
    close(Ks.getH(), Ko.getH(), 1e-12, "Lanczos H of a device-resident Hermitian dense matrix", mat=True)
    Z = torch.as_tensor(S + 1j * (A - A.T), device="cuda")                       # complex Hermitian
    assert eu.MIOperator(Z).ishermitian
    Z[2, 1] += 1e-3
    assert not eu.MIOperator(Z).ishermitian


# ------------------------------------------------------------------ C4 ------------------------------------------------
def c4_inputs(n):
    A = (c2_operator(n) * (1 + 0.25j)).tocsc()
    rng = np.random.default_rng(6)
    u = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return A, u


def test_c4_kiops_complex_full_size(eu):
    """BASELINE configs[3] at its full size (n = 1e6, complex, iop = 2).  The reference has no complex kiops (kiops.jl:89,
    arnoldi.jl:197-200 are Float64-only): the build's extension is checked against the oracle's restatement of the same
    extension (same adaptive decisions, same w) and against the group property exp(-A) exp(A) u = u."""
    n = 1_000_000
    A, u = c4_inputs(n)
    op = eu.MIOperator(A)
    w, st = eu.kiops(1.0, op, u, allow_complex=True, ishermitian=False, opnorm=4.6)
    wo, so = ko.kiops(1.0, A, u, allow_complex=True, ishermitian=False, opnorm=4.6)
    assert st == so, (st, so)
    close(w, wo, 1e-12, "C4 kiops complex n=1e6 vs oracle extension")
    back, _ = eu.kiops(-1.0, op, w[:, 0], allow_complex=True, ishermitian=False, opnorm=4.6)
    # both directions are tol = 1e-7 requests, but m = 15 steps converge far below it for t ||A|| ~ 4.6 (measured 7e-15)
    close(back[:, 0], u, 1e-10, "C4 group property kiops(-1) o kiops(+1)")
    # linearity: a scaled input gives the scaled output with the same decisions
    w3, st3 = eu.kiops(1.0, op, 3.0 * u, allow_complex=True, ishermitian=False, opnorm=4.6)
    close(w3, 3.0 * w, 1e-12, "C4 linearity")


@pytest.mark.parametrize("ncols", [1, 3])
def test_c4_kiops_complex_small_vs_truth_and_oracle(eu, ncols):
    n = 400
    A, u0 = c4_inputs(n)
    rng = np.random.default_rng(16)
    u = u0 if ncols == 1 else np.asfortranarray(np.stack([u0] + [rng.standard_normal(n) * 0.1 * (1 + 1j) for _ in range(ncols - 1)], axis=1))
    w, st = eu.kiops(1.0, A, u, allow_complex=True, ishermitian=False)
    wo, so = ko.kiops(1.0, A, u, allow_complex=True, ishermitian=False)
    assert st == so
    close(w, wo, 1e-12, "C4-style kiops complex small (%d columns) vs oracle" % ncols)
    if ncols == 1:
        close(w[:, 0], sl.expm(A.toarray()) @ u, 1e-6, "C4-style kiops complex vs dense expm (tol 1e-7 method)")


def test_kiops_workspace_is_fresh_per_call(eu):
    """the KrylovSubspace kiops keeps in the context between calls must look like the reference's fresh
    one (kiops.jl:74): same context, different u / iop / Hermitian-ness / rejected steps in between."""
    rng = np.random.default_rng(21)
    n = 500
    ctx = eu.Context()
    A = c2_operator(n).tocsc()
    As = c2_operator(n, sym=True).tocsc()
    op, ops = eu.MIOperator(A, ctx), eu.MIOperator(As, ctx)
    u_big = rng.standard_normal((n, 3)) * 50.0             # long trajectory: rejections, m grows
    u_small = rng.standard_normal((n, 3)) * 1e-3
    seq = [(op, A, u_big, dict(iop=2, tol=1e-10)), (op, A, u_small, dict(iop=5)), (ops, As, u_big, dict(iop=2)),
           (op, A, u_small[:, 0], dict(iop=2, tol=1e-12)), (op, A, u_big, dict(iop=3, m=12)), (op, A, u_small, dict(iop=2))]
    for k, (o, M, u, kw) in enumerate(seq):
        w, st = eu.kiops(2.0, o, u, **kw)
        wo, so = ko.kiops(2.0, M, u, **kw)
        assert st == so, (k, st, so)
        close(w, wo, 1e-12, "kiops call %d on one context vs oracle" % k)


# ------------------------------------------------------------------ C5 ------------------------------------------------
def test_c5_batch_full_problem_size_vs_c_oracle(eu):
    """BASELINE configs[4] at its per-problem size (n = 1e5, m = 30), 16 problems: every column against the plain-C
    restatement of the reference loop run on that problem alone."""
    rng = np.random.default_rng(7)
    n, nprob, m = 100_000, 16, 30
    A0 = c2_operator(n).tocsr()
    A0.sort_indices()
    scales = 1 + 0.1 * rng.random(nprob)
    vals = np.stack([A0.data * s for s in scales])
    B = np.asfortranarray(rng.standard_normal((n, nprob)))
    W, mu = eu.expv_batch(1.0, A0, vals, B, m=m, return_m=True)
    worst = 0.0
    for p in range(nprob):
        Ap = A0.copy()
        Ap.data = vals[p].copy()
        wo, r = co.expv_csr(1.0, Ap, B[:, p], m=m)
        assert mu[p] == r["m"] == m
        worst = max(worst, relerr(W[:, p], wo))
    close(worst, 0.0, 1e-12, "C5 batch n=1e5 x 16, worst column vs C oracle", absolute=True)
    # the batch equals a loop over the single-problem entry point (the reference has no batching: a host `for`)
    for p in (0, nprob - 1):
        Ap = A0.copy()
        Ap.data = vals[p].copy()
        close(W[:, p], eu.expv(1.0, Ap, B[:, p], m=m, ishermitian=False), 1e-13, "C5 batch column %d vs expv()" % p)


# ------------------------------------------------------------------ ADVICE items --------------------------------------
def test_host_matrix_mutated_in_place_is_read_again(eu):
    """mul!(y, A, x) reads A at call time; an implicitly uploaded copy must not go stale."""
    n = 300
    b = np.random.default_rng(2).standard_normal(n)
    A = c2_operator(n).tocsr()
    w1 = eu.expv(1.0, A, b, m=20)
    A.data[:] *= 0.5                                       # typical time-stepping: A .*= dt
    w2 = eu.expv(1.0, A, b, m=20)
    close(w2, ko.expv(1.0, A, b, m=20), 1e-12, "sparse operator after in-place scaling")
    assert relerr(w2, w1) > 1e-3
    D = A.toarray()
    v1 = eu.expv(1.0, D, b, m=20)
    D[0, 0] += 0.25
    close(eu.expv(1.0, D, b, m=20), ko.expv(1.0, D, b, m=20), 1e-12, "dense operator after an in-place entry change")
    ctx2 = eu.Context()
    Ks = eu.KrylovSubspace(np.float64, np.float64, n, 20, 0, ctx2)            # same matrix, another context
    eu.arnoldi_(Ks, A, b, m=20)
    close(Ks.getH(), ko.arnoldi(A, b, m=20).getH(), 1e-12, "operator uploaded per context", mat=True)


def test_malformed_sparse_input_is_an_argument_error(eu):
    """the header promises a status, never a crash."""
    import ctypes as C
    from exponentialutilities_jl_amd import _lib as L
    lib = L.load()
    ctx = eu.default_context()
    n = 4
    vals = np.ones(6)
    h = C.c_void_p()

    def csr(rp, ci, v=vals):
        rp, ci = np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32)
        return lib.expv_mi_op_create_csr(ctx._h, L.F64, n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 4, 0, C.byref(h))

    def csc(cp, rv, v=vals):
        cp, rv = np.asarray(cp, dtype=np.int64), np.asarray(rv, dtype=np.int64)
        return lib.expv_mi_op_create_csc(ctx._h, L.F64, n, cp.ctypes.data, rv.ctypes.data, v.ctypes.data, 1, C.byref(h))

    assert csr([0, 2, 1, 4, 6], [0, 1, 2, 3, 0, 1]) == 2          # non-monotone
    assert csr([1, 2, 3, 4, 6], [0, 1, 2, 3, 0, 1]) == 2          # does not start at the base
    assert csr([0, 1, 2, 3, -1], [0, 1, 2, 3, 0, 1]) == 2         # negative nnz
    assert csr([0, 2, 3, 4, 6], [0, 1, 2, 7, 0, 1]) == 2          # column out of range
    assert csc([1, 3, 2, 5, 7], [1, 2, 3, 4, 1, 2]) == 2
    assert csc([0, 2, 3, 5, 6], [1, 2, 3, 4, 1, 2]) == 2
    assert csc([1, 3, 4, 5, 7], [1, 2, 3, 9, 1, 2]) == 2          # row out of range
    assert lib.expv_mi_op_create_csr(ctx._h, L.F64, n, None, None, None, 4, 0, C.byref(h)) == 2
    assert b"rowptr" in lib.expv_mi_last_error(ctx._h)
    assert csr([0, 2, 3, 4, 6], [0, 1, 2, 3, 0, 1]) == 0          # and the well-formed one still works
    lib.expv_mi_op_destroy(h)


# ------------------------------------------------------------------ single-pass step: complex / augmented / long IOP runs ----
def _path_of(eu, ctx, fn):
    """run fn() and return how the context's factorisations ran (context counters before / after)."""
    c0 = ctx.counters()
    out = fn()
    c1 = ctx.counters()
    return out, {k: c1[k] - c0[k] for k in c1}


@pytest.mark.parametrize("case", ["complex_full_m12", "complex_iop3_m48", "complex_hermitian_lanczos", "real_iop3_m60",
                                  "real_iop5_m100", "complex_iop7_m20"])
def test_single_pass_step_variants_match_oracle(eu, case):
    """The banded single-pass step (pipe.hip) for complex operators (windows <= 15 columns), for incomplete orthogonalisation
    over more than 32 steps (kiops grows m to 128: the window, not m, bounds the register budget) and for the complex
    Hermitian Lanczos recurrence (real coefficients, arnoldi.jl:412-413).  Checked against the oracle AND that the
    factorisation really ran on the single-pass step."""
    rng = np.random.default_rng(77)
    ctx = eu.Context()
    n = 3001
    herm, iop, cplx = False, 0, True
    if case == "complex_full_m12":
        m = 12
    elif case == "complex_iop3_m48":
        m, iop = 48, 3
    elif case == "complex_iop7_m20":
        m, iop = 20, 7
    elif case == "complex_hermitian_lanczos":
        m, herm = 30, True
    elif case == "real_iop3_m60":
        m, iop, cplx = 60, 3, False
    else:
        m, iop, cplx = 100, 5, False
    offs = [-2, -1, 0, 1, 2]
    diags = [rng.standard_normal(n - abs(o)) * 0.3 + (1j * rng.standard_normal(n - abs(o)) * 0.2 if cplx else 0) - (2.0 if o == 0 else 0)
             for o in offs]
    A = sp.diags(diags, offs, shape=(n, n), format="csr")
    if herm:
        A = ((A + A.conj().T) * 0.5).tocsr()
    b = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    op = eu.MIOperator(A, ctx)
    T = np.complex128 if cplx else np.float64
    Ks = eu.KrylovSubspace(T, np.float64 if herm else T, n, m, 0, ctx)
    _, path = _path_of(eu, ctx, lambda: eu.arnoldi_(Ks, op, b, m=m, iop=iop, ishermitian=herm))
    assert path["pipeline"] == 1 and path["krylov_steps"] == m, path
    Ko = ko.KrylovSubspace(T, float if herm else T, n, m)
    ko.arnoldi_(Ko, A, b, m=m, iop=iop, ishermitian=herm)
    assert Ks.m == Ko.m and Ks.wasbreakdown == Ko.wasbreakdown
    tol = 1e-12        # (measured <= 4e-13 on every case, IOP windows included: profiles/r02_parity_measured.txt)
    close(Ks.getH(), Ko.getH(), tol, "single-pass step %s: H vs oracle" % case, mat=True)
    close(Ks.getV(), Ko.getV(), tol, "single-pass step %s: V vs oracle (max abs)" % case, absolute=True)
    t = 0.3 - 0.1j if cplx else 0.3
    w = eu.expv_(np.empty(n, dtype=complex if cplx else float), t, Ks)
    close(w, ko.expv_(np.empty(n, dtype=complex if cplx else float), t, Ko), tol, "single-pass step %s: expv! vs oracle" % case)
    if not iop:
        wc, pc = _path_of(eu, ctx, lambda: eu.expv(t, op, b, m=m, ishermitian=herm))           # whole-call form (mailbox, no tail)
        assert pc["pipeline"] == 1
        close(wc, w, 1e-13, "single-pass step %s: whole-call expv vs arnoldi! + expv!" % case)


def test_single_pass_step_continuation_and_augmented_bitwise_forms(eu):
    """(i) arnoldi!(...; init = j) continues on the single-pass step from un-normalised columns + scales and gives what a
    from-scratch factorisation gives; (ii) kiops on a banded operator (augmented operator [A B; 0 K], real and complex)
    runs on it, overlapped and one-launch-after-the-other bit for bit alike."""
    rng = np.random.default_rng(5)
    ctx = eu.Context()
    n = 4000
    A = c2_operator(n)
    op = eu.MIOperator(A, ctx)
    b = rng.standard_normal(n)
    for m0, m1, iop in ((8, 24, 0), (10, 40, 4), (5, 31, 0)):
        Ks = eu.KrylovSubspace(np.float64, np.float64, n, m1, 0, ctx)
        eu.arnoldi_(Ks, op, b, m=m0, iop=iop, ishermitian=False)
        _, path = _path_of(eu, ctx, lambda: eu.arnoldi_(Ks, op, b, m=m1, iop=iop, init=m0, ishermitian=False))
        assert path["pipeline"] == 1 and path["krylov_steps"] == m1 - m0 + 1, path
        Kf = eu.KrylovSubspace(np.float64, np.float64, n, m1, 0, ctx)
        eu.arnoldi_(Kf, op, b, m=m1, iop=iop, ishermitian=False)
        close(Ks.getH(), Kf.getH(), 1e-13, "continuation %d -> %d (iop %d): H vs from scratch" % (m0, m1, iop), mat=True)
        close(Ks.getV(), Kf.getV(), 1e-13, "continuation %d -> %d (iop %d): V vs from scratch (max abs)" % (m0, m1, iop), absolute=True)
        Ko = ko.KrylovSubspace(float, float, n, m1)
        ko.arnoldi_(Ko, A, b, m=m1, iop=iop, ishermitian=False)
        close(Ks.getH(), Ko.getH(), 1e-12, "continuation %d -> %d (iop %d): H vs oracle" % (m0, m1, iop), mat=True)
    for cplx in (False, True):
        Ac = (A * (1 + 0.25j)).tocsr() if cplx else A
        opc = eu.MIOperator(Ac, ctx)
        u = rng.standard_normal((n, 3)) * 30.0 + (1j * rng.standard_normal((n, 3)) if cplx else 0)
        res = []
        for overlap in (True, False):
            ctx.set_pipeline_overlap(overlap)
            (w, st), path = _path_of(eu, ctx, lambda: eu.kiops(1.5, opc, u, allow_complex=cplx, ishermitian=False, tol=1e-9))
            assert path["pipeline"] == path["factorisations"] >= 2, path        # every factorisation (fresh and continued)
            res.append((np.asarray(w).copy(), st))
        ctx.set_pipeline_overlap(True)
        assert res[0][1] == res[1][1] and np.array_equal(res[0][0], res[1][0])
        wo, so = ko.kiops(1.5, Ac, u, allow_complex=cplx, ishermitian=False, tol=1e-9)
        assert res[0][1] == so
        close(res[0][0], wo, 1e-12, "kiops on the single-pass step (complex=%s) vs oracle" % cplx)


def test_batch_over_several_contexts_from_one_process(eu):
    """expv_mi_expv_batch_multi (the Julia host's way to run config 5): shards over contexts, one host thread per shard,
    final gather into a host matrix or into ctxs[0]'s device matrix.  One GPU here, so the contexts share device 0 -- the
    sharding, threading and gather code is the same."""
    rng = np.random.default_rng(17)
    n, nprob, m = 20_000, 7, 30
    A0 = c2_operator(n).tocsr()
    A0.sort_indices()
    vals = np.stack([A0.data * s for s in 1 + 0.1 * rng.random(nprob)])
    B = np.asfortranarray(rng.standard_normal((n, nprob)))
    ts = np.linspace(0.5, 1.0, nprob)
    ref, mref = eu.expv_batch(ts, A0, vals, B, m=m, return_m=True)
    for nctx in (1, 2, 3):
        ctxs = [eu.Context() for _ in range(nctx)]
        W, mu = eu.expv_batch_multi(ts, A0, vals, B, ctxs, m=m, return_m=True)
        close(W, ref, 1e-15, "batch over %d context(s), host gather, vs single-context batch" % nctx)
        assert np.array_equal(mu, mref)
        Wd = eu.DeviceArray((n, nprob), np.float64, ctxs[0])
        eu.expv_batch_multi(ts, A0, vals, B, ctxs, m=m, out=Wd)
        close(Wd.to_host(), ref, 1e-15, "batch over %d context(s), device gather (peer copies)" % nctx)
    with pytest.raises(eu.DimensionMismatch):
        eu.expv_batch_multi(ts, A0, vals[:, :-1], B, [eu.Context()], m=m)


def test_c_abi_rccl_gather_world_size_one(eu):
    """north_star: "RCCL over xGMI for the final gather only".  The C ABI's own gather (expv_mi_comm_create / expv_mi_gather_rccl:
    librccl.so through dlopen, ncclAllGather on the context's stream) -- what a Julia host with one process per GPU calls, without
    torch.distributed.  RCCL refuses two ranks on ONE device, so a 1-GPU box can only run world size 1: communicator creation from a
    unique id, the gather of a batch's result block enqueued BEHIND the batch on the same stream (stream-ordered outputs: no host
    synchronisation in between), every element type as bytes, destroy.  The 2-rank form is the same call with nranks = 2."""
    import torch
    assert eu.rccl_available(), "librccl.so must load on the GPU box"
    ctx = eu.Context(async_outputs=True)
    uid = eu.rccl_unique_id()
    assert len(uid) == 128 and any(uid)
    comm = eu.RcclComm(ctx, uid, 1, 0)
    rng = np.random.default_rng(23)
    n, nprob, m = 20_000, 5, 30
    A0 = c2_operator(n).tocsr()
    A0.sort_indices()
    vals = np.stack([A0.data * s for s in 1 + 0.1 * rng.random(nprob)])
    B = np.asfortranarray(rng.standard_normal((n, nprob)))
    ts = np.linspace(0.5, 1.0, nprob)
    ref = eu.expv_batch(ts, A0, vals, B, m=m, ctx=eu.Context())
    Wd = eu.DeviceArray((n, nprob), np.float64, ctx)
    eu.expv_batch_multi(ts, A0, vals, B, [ctx], m=m, out=Wd)                 # this rank's block, left on its device
    recv = eu.DeviceArray((n, nprob), np.float64, ctx)
    comm.all_gather_raw(Wd.ptr, recv.ptr, n * nprob, np.float64)            # (no ctx.sync() in between)
    ctx.sync()
    got = recv.to_host()
    close(got, np.asarray(ref), 1e-15, "C-ABI RCCL all-gather of a batch's result block (world size 1) vs the single-context batch")
    for dt in (torch.float32, torch.complex64, torch.complex128):
        x = torch.randn(3001, dtype=dt, device="cuda")
        torch.cuda.synchronize()
        y = comm.all_gather(x)
        ctx.sync()
        assert torch.equal(x, y), dt
    comm.destroy()
    with pytest.raises(ValueError):
        eu.RcclComm(ctx, b"short", 1, 0)


def test_basis_reuse_across_tau_only_retries_is_bit_identical(eu):
    """phiv_timestep! rebuilds the Krylov basis on every adaptation retry
    (krylov_phiv_adaptive.jl:417) even when only tau changed; the basis does not depend on tau, so the build keeps it.
    Same controller decisions and statistics as the oracle, results bit-identical to the rebuild-every-time form."""
    # (the long n = 600 run -- 12 sub-steps at t ||A|| ~ 1300, m = 80 -- sits on a ceil() boundary of the m-controller: device
    #  and oracle error estimates differ in the 7th digit there and pick m = 86 / 87; it is kept for the bitwise comparison of
    #  the two forms of the build only)
    for n, m, t, tol, nb, vs_oracle in ((600, 80, 300.0, 1e-8, 3, False), (300, 60, 60.0, 1e-9, 3, True), (400, 70, 120.0, 1e-9, 2, True),
                                        (500, 90, 200.0, 1e-10, 3, True)):
        rng = np.random.default_rng(14)
        A = c2_operator(n).tocsc()
        B = np.asfortranarray(rng.standard_normal((n, nb)))
        op = eu.MIOperator(A)
        s_re, s_no, so = {}, {}, {}
        U_re = eu.phiv_timestep(np.array([t / 3, t]), op, B, adaptive=True, tol=tol, m=m, stats=s_re)
        U_no = eu.phiv_timestep(np.array([t / 3, t]), op, B, adaptive=True, tol=tol, m=m, stats=s_no, reuse_basis=False)
        Uo = ko.phiv_timestep(np.array([t / 3, t]), A, B, adaptive=True, tol=tol, m=m, stats=so)
        assert s_re["arnoldi_reused"] >= 1 and s_no["arnoldi_reused"] == 0, (s_re, s_no)
        for k in ("num_timesteps", "matvecs", "m", "arnoldi_calls"):
            assert s_re[k] == s_no[k], (k, s_re, s_no)
        assert np.array_equal(np.asarray(U_re), np.asarray(U_no))
        if vs_oracle:
            assert (s_re["num_timesteps"], s_re["matvecs"], s_re["m"]) == (so["num_timesteps"], so["matvecs"], so["m"]), (s_re, so)
            close(U_re, Uo, 1e-12, "phiv_timestep with basis reuse (n=%d m=%d t=%g, %d tau-only retries) vs oracle" % (n, m, t, s_re["arnoldi_reused"]))


@pytest.mark.parametrize("T", [np.float32, np.complex64])
def test_32bit_operands_follow_the_reference_result_type(eu, T):
    """Float32 / ComplexF32 operands: the reference computes and returns in that type (BlasFloat, ExponentialUtilities.jl:19);
    the build promotes to fp64 on upload, computes there and rounds the result of expv to the reference's promote_type."""
    rng = np.random.default_rng(3)
    n = 200
    A = (c2_operator(n).toarray() * (1 + (0.25j if np.dtype(T).kind == "c" else 0))).astype(T)
    b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(T).kind == "c" else 0)).astype(T)
    w = eu.expv(0.5, A, b, m=30)
    assert w.dtype == np.dtype(T)
    truth = sl.expm(0.5 * A.astype(np.complex128)) @ b.astype(np.complex128)
    close(w.astype(np.complex128), truth, 2e-6, "expv with %s operands vs dense truth (fp32 rounding of inputs and result)" % np.dtype(T).name)
    w64 = eu.expv(0.5, A.astype(np.complex128 if np.dtype(T).kind == "c" else np.float64), b, m=30)
    assert w64.dtype.itemsize == 2 * np.dtype(T).itemsize
    # promote_type(typeof(t), eltype(A), eltype(b)): a Float64 t (numpy scalar) with 32-bit operands gives the 64-bit type,
    # a literal takes the operands' precision -- in every front end
    assert eu.expv(np.float64(0.5), A, b, m=30).dtype.itemsize == 2 * np.dtype(T).itemsize
    assert eu.phiv(0.5, A, b, 2, m=20).dtype == np.dtype(T)
    assert eu.phiv(np.float64(0.5), A, b, 2, m=20).dtype.itemsize == 2 * np.dtype(T).itemsize
    if np.dtype(T).kind == "f":
        As = ((A + A.T) / 2).astype(T)
        assert eu.expv(0.5, As, b, m=30, mode="error_estimate").dtype == np.dtype(T)
    assert eu.expv.last_stats["path"]                              # (dense: modular launches; sparse banded: the single-pass step)
    # a Python complex t is a Complex in promote_type whatever its imaginary part -- expv(1 + 0im, A, b) is complex
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wc = eu.expv(0.5 + 0j, A, b, m=30)
        pc = eu.phiv(0.5 + 0j, A, b, 1, m=20)
    assert wc.dtype == np.dtype(np.complex64) and pc.dtype == np.dtype(np.complex64)
    close(wc.astype(np.complex128), truth, 2e-6, "expv with t = 0.5 + 0j and %s operands: complex result" % np.dtype(T).name)
    assert eu.expv(0.5 + 0j, A.astype(np.float64 if np.dtype(T).kind == "f" else np.complex128), b.astype(np.float64 if np.dtype(T).kind == "f" else np.complex128), m=30).dtype == np.dtype(np.complex128)


@pytest.mark.parametrize("T", [np.float32, np.complex64])
@pytest.mark.parametrize("kind", ["sparse_banded", "sparse_irregular", "dense"])
def test_native_32bit_krylov_path(eu, T, kind):
    """Float32 / ComplexF32 natively on the device (ExponentialUtilities.jl:19 BlasFloat,
    test/basictests.jl:952-974): 32-bit storage (4 / 2 rows per 16-byte pack), fp64 projection sums, the two-kernel step and the
    modular launches.  Against the fp64 oracle on the same (fp32-representable) inputs at fp32 bars: H and V of arnoldi!, expv,
    phiv, mul!, strict MGS and low-sync, Lanczos on a Hermitian operator, the error-estimate mode and phiv_timestep!."""
    from tests.test_gpu_parity import powerlaw_matrix
    cplx = np.dtype(T).kind == "c"
    rng = np.random.default_rng(41)
    n, m = 3000, 20
    if kind == "sparse_banded":
        A = (c2_operator(n) * (1 + (0.25j if cplx else 0))).astype(T).tocsr()
    elif kind == "sparse_irregular":
        A = powerlaw_matrix(n, 5, cplx=cplx).astype(T).tocsr()
    else:
        n = 700
        A = (-0.5 * np.eye(n) + (rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)) / np.sqrt(n)).astype(T)
    b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)).astype(T)
    A64 = A.astype(np.complex128 if cplx else np.float64)
    b64 = b.astype(np.complex128 if cplx else np.float64)
    op = eu.MIOperator(A)
    assert op.dtype == np.dtype(T)
    x = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)).astype(T)
    y = op @ x
    assert np.asarray(y).dtype == np.dtype(T)
    close(np.asarray(y).astype(A64.dtype), A64 @ x.astype(A64.dtype), 5e-6, "mul! %s %s (fp32 bar)" % (np.dtype(T).name, kind))
    # the oracle run IN the 32-bit type (numpy float32 / complex64 arithmetic end to end: what the reference's
    # own BlasFloat methods compute) sets the scale of the bars -- its distance to the fp64 oracle is the error of pure 32-bit
    # arithmetic on this problem, and the device (32-bit storage, fp64 sums) has to stay within a small multiple of it
    K32 = ko.arnoldi(A, b, m=m, ishermitian=False)
    assert K32.getH().dtype == np.dtype(T)
    for ortho in ("lowsync", "mgs"):
        Ks = eu.arnoldi(op, b, m=m, ishermitian=False, ortho=ortho)
        Ko = ko.arnoldi(A64, b64, m=m, ishermitian=False)
        assert Ks.T == np.dtype(T) and Ks.m == Ko.m == K32.m and Ks.getH().dtype == np.dtype(T)
        eH = close(Ks.getH().astype(A64.dtype), Ko.getH(), 2e-5, "arnoldi H %s %s %s vs the fp64 oracle (fp32 bar)" % (np.dtype(T).name, kind, ortho), mat=True)
        eV = close(Ks.getV().astype(A64.dtype), Ko.getV(), 2e-5, "arnoldi V %s %s %s vs the fp64 oracle (max abs, fp32 bar)" % (np.dtype(T).name, kind, ortho), absolute=True)
        rH = close(K32.getH().astype(A64.dtype), Ko.getH(), 2e-5, "  the oracle in %s arithmetic vs the fp64 oracle: H" % np.dtype(T).name, mat=True)
        rV = close(K32.getV().astype(A64.dtype), Ko.getV(), 2e-5, "  the oracle in %s arithmetic vs the fp64 oracle: V (max abs)" % np.dtype(T).name, absolute=True)
        close(Ks.getH().astype(A64.dtype), K32.getH().astype(A64.dtype), 2e-5, "arnoldi H %s %s %s vs the oracle in %s arithmetic" % (np.dtype(T).name, kind, ortho, np.dtype(T).name), mat=True)
        assert eH <= 20 * rH + 1e-7 and eV <= 20 * rV + 1e-7, (eH, rH, eV, rV)
    w = eu.expv(0.7, op, b, m=m, ishermitian=False)
    assert np.asarray(w).dtype == np.dtype(T)
    close(np.asarray(w).astype(A64.dtype), ko.expv(0.7, A64, b64, m=m, ishermitian=False), 1e-5, "expv %s %s (fp32 bar)" % (np.dtype(T).name, kind))
    W = eu.phiv(0.5, op, b, 2, m=m)
    assert np.asarray(W).dtype == np.dtype(T)
    close(np.asarray(W).astype(A64.dtype), ko.phiv(0.5, A64, b64, 2, m=m), 2e-5, "phiv %s %s (fp32 bar)" % (np.dtype(T).name, kind))
    # complex time on 32-bit operands: ComplexF32 result
    wc = eu.expv(0.3 - 0.4j, op, b, m=m, ishermitian=False)
    assert np.asarray(wc).dtype == np.dtype(np.complex64)
    close(np.asarray(wc).astype(np.complex128), ko.expv(0.3 - 0.4j, A64, b64, m=m, ishermitian=False), 1e-5,
          "expv complex t %s %s (fp32 bar)" % (np.dtype(T).name, kind))
    if kind != "sparse_irregular":
        # Hermitian operator: lanczos!, U = Float32, and the error-estimate mode
        Ah = ((A64 + A64.conj().T) * 0.5)
        Ah = Ah.astype(T) if kind == "dense" else Ah.astype(T).tocsr()
        Ah64 = Ah.astype(A64.dtype)
        Kh = eu.arnoldi(Ah, b, m=m)
        assert Kh.U == np.dtype(np.float32) and Kh.getH().dtype == np.dtype(np.float32)
        Kho = ko.arnoldi(Ah64, b64, m=m)
        close(Kh.getH().astype(np.float64), np.real(Kho.getH()), 2e-5, "lanczos H %s %s (fp32 bar)" % (np.dtype(T).name, kind), mat=True)
        we = eu.expv(0.7, Ah, b, m=m, mode="error_estimate", rtol=1e-4)
        assert np.asarray(we).dtype == np.dtype(T)
        truth = sl.expm(0.7 * (Ah64.toarray() if hasattr(Ah64, "toarray") else Ah64)) @ b64
        close(np.asarray(we).astype(A64.dtype), truth, 5e-4, "expv error_estimate %s %s (rtol 1e-4)" % (np.dtype(T).name, kind))
    # phiv_timestep!, adaptive
    B = (rng.standard_normal((n, 3)) + (1j * rng.standard_normal((n, 3)) if cplx else 0)).astype(T)
    U = eu.phiv_timestep(np.array([0.4, 1.0]), op, B, adaptive=True, tol=1e-5)
    assert np.asarray(U).dtype == np.dtype(T)
    Uo = ko.phiv_timestep(np.array([0.4, 1.0]), A64, B.astype(A64.dtype), adaptive=True, tol=1e-5)
    close(np.asarray(U).astype(A64.dtype), Uo, 2e-4, "phiv_timestep %s %s (tol 1e-5, fp32 bar)" % (np.dtype(T).name, kind))
    # the 64-bit-only entry points say so through the C ABI; the Python mirrors promote (kiops: Float64 reference method)
    if not cplx:
        wk, st = eu.kiops(0.5, A, B)
        assert np.asarray(wk).dtype == np.float64


def test_context_options_select_the_step_form(eu):
    """Engine switches are context options (expv_mi_ctx_set_option), not process environment: the same operator and vector
    through the three step forms give the same result, and the context reports which one ran."""
    n, m = 30_000, 20
    A = c2_operator(n)
    b = np.random.default_rng(2).standard_normal(n)
    wo = ko.expv(0.8, A, b, m=m, ishermitian=False)
    ctx = eu.Context()
    op = eu.MIOperator(A, ctx)
    assert ctx.get_option("pipeline") == 1 and ctx.get_option("spin_limit") == 400000
    seen = []
    for opts, want in (({}, "pipeline"), ({"pipeline": 0}, "two_kernel"), ({"pipeline": 0, "fused": 0}, "modular"),
                       ({"pipeline": 0, "dia": 0}, "two_kernel"), ({"pipeline": 0, "fused_two_reductions": 1}, "two_kernel"),
                       ({"mailbox": 0}, "pipeline"), ({"pipeline_serial": 1}, "pipeline")):
        for k in ("pipeline", "fused", "dia", "mailbox"):
            ctx.set_option(k, 1)
        for k in ("fused_two_reductions", "pipeline_serial"):
            ctx.set_option(k, 0)
        for k, v in opts.items():
            ctx.set_option(k, v)
        w = eu.expv(0.8, op, b, m=m, ishermitian=False)
        path = eu.expv.last_stats["path"]
        assert want in path, (opts, path)
        assert ("overlapped" in path) == (want == "pipeline" and not opts.get("pipeline_serial")), (opts, path)
        close(w, wo, 1e-12, "expv through options %s (%s)" % (opts, "+".join(path)))
        seen.append(path)
    with pytest.raises(eu.ExpvMIError):
        ctx.set_option("no_such_option", 1)
    c = ctx.counters()
    assert c["redo_serial"] == 0 and c["redo_wave_off"] == 0 and c["factorisations"] == len(seen)


def test_resident_form_matches_stepwise_and_oracle(eu):
    """Context option "resident" = 1: the whole factorisation as one cooperative kernel (pipe.hip, k_pipe_resident).  Same
    algorithm as the step-wise single-pass form with another partition of the rows: agreement to rounding with it and with
    the C oracle, happy breakdown included, and the path flag says that it ran."""
    rng = np.random.default_rng(77)
    for n, m in ((200_000, 30), (70_001, 12)):
        A = c2_operator(n)
        b = rng.standard_normal(n)
        ctx = eu.Context()
        op = eu.MIOperator(A, ctx)
        w_step = eu.expv(0.7, op, b, m=m, ishermitian=False)
        assert "resident" not in eu.expv.last_stats["path"]
        ctx.set_option("resident", 1)
        w_res = eu.expv(0.7, op, b, m=m, ishermitian=False)
        assert "resident" in eu.expv.last_stats["path"], eu.expv.last_stats
        w_ref, _ = co.expv_csr(0.7, A, b, m=m)
        close(w_res, w_step, 1e-13, "resident form vs step-wise form (n=%d, m=%d)" % (n, m))
        close(w_res, w_ref, 1e-12, "resident form vs C oracle (n=%d, m=%d)" % (n, m))
    # happy breakdown inside the resident kernel: b is a combination of 8 eigenvectors of a tridiagonal Toeplitz operator
    # (full diagonals, so the operator takes the DIA form the resident kernel needs)
    n = 4096
    A = sp.diags([0.5, 1.5, 0.5], [-1, 0, 1], shape=(n, n), format="csc")
    i = np.arange(1, n + 1)
    b = sum((1.0 + 1e-3 * k) * np.sin(np.pi * k * i / (n + 1)) / 64.0 for k in (300, 800, 1300, 1800, 2300, 2800, 3300, 3800))
    ctx = eu.Context()
    ctx.set_option("resident", 1)
    op = eu.MIOperator(A, ctx)
    w = eu.expv(0.3, op, b, m=20, ishermitian=False)
    st = dict(eu.expv.last_stats)
    assert "resident" in st["path"] and st["wasbreakdown"] and st["m"] <= 9, st
    lam = 1.5 + np.cos(np.pi * np.array([300, 800, 1300, 1800, 2300, 2800, 3300, 3800]) / (n + 1))
    w_exact = sum(np.exp(0.3 * l) * (1.0 + 1e-3 * k) * np.sin(np.pi * k * i / (n + 1)) / 64.0
                  for l, k in zip(lam, (300, 800, 1300, 1800, 2300, 2800, 3300, 3800)))
    close(w, w_exact, 1e-10, "resident form, happy breakdown")


def test_nontemporal_loads_change_nothing_but_the_cache_policy(eu):
    """Context option "nontemporal" (-1: by the footprint of a step, 0 never, 1 always): the single-pass step reads the window
    columns and operator diagonals with non-temporal loads when a step's footprint is far beyond the Infinity Cache.  Only the
    cache policy of the loads differs: results are bitwise equal, for the single problem (overlapped and serial) and the batch."""
    n, m = 60_000, 24
    A = c2_operator(n)
    b = np.random.default_rng(5).standard_normal(n)
    res = {}
    for nt in (0, 1):
        for serial in (0, 1):
            ctx = eu.Context()
            ctx.set_option("nontemporal", nt)
            ctx.set_option("pipeline_serial", serial)
            op = eu.MIOperator(A, ctx)
            res[(nt, serial)] = eu.expv(0.9, op, b, m=m, ishermitian=False)
            assert "pipeline" in eu.expv.last_stats["path"]
    assert np.array_equal(res[(0, 0)], res[(1, 0)]) and np.array_equal(res[(0, 1)], res[(1, 1)])
    A0 = A.tocsr(); A0.sort_indices()
    vals = np.stack([A0.data * s for s in (1.0, 1.05, 0.97)])
    B = np.asfortranarray(np.random.default_rng(6).standard_normal((n, 3)))
    B[:, 0] = b
    W = []
    for nt in (0, 1):
        ctx = eu.Context()
        ctx.set_option("nontemporal", nt)
        W.append(np.asarray(eu.expv_batch(0.9, A0, vals, B, m=m, ctx=ctx)))
    assert np.array_equal(W[0], W[1])
    close(W[0][:, 0], res[(0, 1)], 1e-13, "batch column 0 vs single expv (nontemporal test)")


def test_constant_coefficient_stencil_option_is_bitwise_neutral(eu):
    """Context option "stencil" = 1: a banded operator whose stored diagonals are constant (constant-coefficient finite
    differences) is applied from scalars instead of streamed diagonals.  Same products in the same order: results are
    bitwise equal to the general DIA path, overlapped and serial, ragged size included; an operator that is NOT constant
    along its diagonals takes the general path unchanged."""
    rng = np.random.default_rng(99)
    for n, m in ((100_003, 30), (7_001, 12)):
        A = c2_operator(n)
        b = rng.standard_normal(n)
        res = {}
        for stencil in (0, 1):
            for serial in (0, 1):
                ctx = eu.Context()
                ctx.set_option("stencil", stencil)
                ctx.set_option("pipeline_serial", serial)
                op = eu.MIOperator(A, ctx)
                Ks = eu.KrylovSubspace(np.float64, np.float64, n, m, 0, ctx)
                eu.arnoldi_(Ks, op, b, m=m, ishermitian=False)
                res[(stencil, serial)] = (Ks.H.copy(), Ks.getV().copy(), np.asarray(eu.expv(0.6, op, b, m=m, ishermitian=False)).copy())
        for serial in (0, 1):
            for x0, x1 in zip(res[(0, serial)], res[(1, serial)]):
                assert np.array_equal(x0, x1), (n, m, serial)
        wo, _ = co.expv_csr(0.6, A, b, m=m)
        close(res[(1, 0)][2], wo, 1e-12, "stencil option vs C oracle (n=%d, m=%d)" % (n, m))
    # not constant along the diagonals: same pattern, one entry changed
    n = 20_000
    A = c2_operator(n).tolil()
    A[5000, 5001] = 0.75
    A = A.tocsc()
    b = rng.standard_normal(n)
    w = []
    for stencil in (0, 1):
        ctx = eu.Context()
        ctx.set_option("stencil", stencil)
        w.append(np.asarray(eu.expv(0.6, eu.MIOperator(A, ctx), b, m=20, ishermitian=False)))
    assert np.array_equal(w[0], w[1])
    close(w[1], co.expv_csr(0.6, A, b, m=20)[0], 1e-12, "stencil option on a non-constant operator vs C oracle")


def test_row_sharded_dense_operator_on_the_device(eu):
    """dist.RowShardedDense at world size 1 (the multi-rank exchange is covered by the gloo test on CPU): the adaptive
    phiv_timestep driven by the sharded matrix-free operator takes the controller decisions of the dense operator path and
    gives the same snapshots."""
    import importlib.util, os, torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mi_dist", os.path.join(root, "exponentialutilities.jl_amd", "dist.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    n = 1500
    A, B = c3_inputs(n)
    ctx = eu.Context()
    sh = D.RowShardedDense(D.RowShardedDense.column_major(torch.as_tensor(np.ascontiguousarray(A), device="cuda")), n)
    op = sh.operator(eu, ctx)
    st, sd = {}, {}
    ts = np.array([3.0, 12.0, 7.5])
    U = eu.phiv_timestep(ts.copy(), op, B, adaptive=True, tol=1e-9, stats=st)
    Ud = eu.phiv_timestep(ts.copy(), eu.MIOperator(A, ctx), B, adaptive=True, tol=1e-9, stats=sd)
    assert (st["num_timesteps"], st["matvecs"], st["m"]) == (sd["num_timesteps"], sd["matvecs"], sd["m"]), (st, sd)
    assert sh.applications >= st["matvecs"]
    close(U, Ud, 1e-12, "phiv_timestep through the row-sharded operator vs the dense operator (n=%d)" % n)


@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.complex128])
def test_row_sharded_dense_operator_passes_its_own_element_type(eu, dtype):
    """RowShardedDense handed every block to expv_mi_gemv_block as fp64 / complex-fp64; a Float32 /
    ComplexF32 block (which operator() creates natively in that type) was read as 8 / 16-byte elements.  mul! and expv through the
    sharded operator (world size 1) against numpy / the dense operator of the same type, at a size that takes the column-split
    form."""
    import importlib.util, os, torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mi_dist", os.path.join(root, "exponentialutilities.jl_amd", "dist.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    n = 1300
    rng = np.random.default_rng(17)
    A = (rng.standard_normal((n, n)) / np.sqrt(n)).astype(dtype)
    x = rng.standard_normal(n).astype(dtype)
    if np.dtype(dtype).kind == "c":
        A = (A + 1j * rng.standard_normal((n, n)) / np.sqrt(n)).astype(dtype)
        x = (x + 1j * rng.standard_normal(n)).astype(dtype)
    ctx = eu.Context()
    sh = D.RowShardedDense(D.RowShardedDense.column_major(torch.as_tensor(np.ascontiguousarray(A), device="cuda")), n)
    assert sh._nsplit > 1
    op = sh.operator(eu, ctx)
    assert op.dtype == np.dtype(dtype)
    tol = 2e-5 if np.dtype(dtype).itemsize <= 8 else 1e-13
    y = np.asarray(op.matvec(x))
    close(y, A.astype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64) @ x, tol, "row-sharded mul! %s vs numpy" % np.dtype(dtype).name)
    w = np.asarray(eu.expv(0.7, op, x, m=12))
    wd = np.asarray(eu.expv(0.7, eu.MIOperator(A, ctx), x, m=12))
    assert w.dtype == wd.dtype
    close(w, wd, tol, "expv through the row-sharded %s operator vs the dense operator" % np.dtype(dtype).name)
    with pytest.raises(TypeError):
        sh._local_gemv(torch.zeros(n, dtype=torch.float64 if dtype != np.float64 else torch.float32, device="cuda")
                       if dtype != np.complex128 else torch.zeros(n, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
@pytest.mark.parametrize("shape", [(1, 7), (63, 200), (700, 1500), (1201, 64), (513, 513)])
def test_gemv_block_rectangular(eu, dtype, shape):
    """expv_mi_gemv_block: y = A x for a device-resident column-major nrows x ncols block (the local half of the row-sharded
    config-3 operator), single launch and column-split form, against numpy."""
    import ctypes as C
    import torch
    from exponentialutilities_jl_amd import _lib as L
    nr, nc = shape
    rng = np.random.default_rng(nr * 1000 + nc)
    A = rng.standard_normal((nr, nc)).astype(dtype)
    x = rng.standard_normal(nc).astype(dtype)
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.standard_normal((nr, nc))
        x = x + 1j * rng.standard_normal(nc)
    ctx = eu.Context()
    Ad = torch.as_tensor(np.ascontiguousarray(A.T), device="cuda").t()          # column-major nr x nc
    xd = torch.as_tensor(x, device="cuda")
    torch.cuda.synchronize()
    ref = A @ x
    for nsplit in (1, 5):
        yd = torch.zeros(nr, dtype=xd.dtype, device="cuda")
        scr = torch.empty(nsplit * nr, dtype=xd.dtype, device="cuda")
        torch.cuda.synchronize()
        rc = L.load().expv_mi_gemv_block(ctx._h, 1 if np.dtype(dtype).kind == "c" else 0, nr, nc, Ad.data_ptr(), Ad.stride(1) if nc > 1 else nr,
                                         xd.data_ptr(), yd.data_ptr(), scr.data_ptr() if nsplit > 1 else None, nsplit)
        assert rc == 0
        ctx.sync()
        close(yd.cpu().numpy(), ref, 1e-13, "gemv_block %dx%d %s nsplit=%d vs numpy" % (nr, nc, np.dtype(dtype).name, nsplit))


def _rows_worker(rank, world, port, n, out_dir):
    import os, sys, importlib.util
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import torch.distributed as dist
    import expv_mi_loader
    eu = expv_mi_loader.load()
    spec = importlib.util.spec_from_file_location("mi_dist", os.path.join(root, "exponentialutilities.jl_amd", "dist.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        A, B = c3_inputs(n)
        lo, hi = D.shard_range(n, world, rank)
        # both ranks share the one GPU of the test box; gloo has no device all-gather, so the pieces are staged through the host
        sh = D.RowShardedDense(D.RowShardedDense.column_major(torch.as_tensor(np.ascontiguousarray(A[lo:hi]), device="cuda")), n, stage_through_host=True)
        st = {}
        U = eu.phiv_timestep(np.array([3.0, 7.5]), sh.operator(eu, eu.Context()), B, adaptive=True, tol=1e-9, stats=st)
        np.save(os.path.join(out_dir, "U_%d.npy" % rank), np.asarray(U))
        np.save(os.path.join(out_dir, "st_%d.npy" % rank), np.array([st["num_timesteps"], st["matvecs"], st["m"], sh.applications]))
    finally:
        dist.destroy_process_group()


def test_row_sharded_dense_operator_two_processes_one_gpu(eu, tmp_path):
    """Two processes (gloo, both on the test box's single GPU), each holding half of the rows of the config-3 operator: the
    device engine of each process drives the all-gather from inside its operator callback; both replicas take the same
    sub-steps and end with the same snapshots as the unsharded dense operator."""
    import socket
    import torch.multiprocessing as mp
    n, world = 1200, 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_rows_worker, args=(world, port, n, str(tmp_path)), nprocs=world, join=True)
    A, B = c3_inputs(n)
    sd = {}
    Ud = np.asarray(eu.phiv_timestep(np.array([3.0, 7.5]), A, B, adaptive=True, tol=1e-9, stats=sd))
    U0, U1 = np.load(tmp_path / "U_0.npy"), np.load(tmp_path / "U_1.npy")
    s0, s1 = np.load(tmp_path / "st_0.npy"), np.load(tmp_path / "st_1.npy")
    assert np.array_equal(U0, U1) and np.array_equal(s0, s1)
    assert tuple(s0[:3]) == (sd["num_timesteps"], sd["matvecs"], sd["m"]), (s0, sd)
    close(U0, Ud, 1e-12, "row-sharded operator, 2 processes on one GPU, vs the dense operator (n=%d)" % n)


@pytest.mark.gpu
def test_device_selftest_lane_exchanges_match_the_lds_permute_forms(eu):
    """kernel_common.h sums across a wave with v_permlane32/16_swap + DPP; the C ABI's self-test runs every such routine
    against its __shfl_xor (ds_bpermute) form on random values and counts lanes that differ in any bit."""
    ctx = eu.Context()
    assert ctx.selftest() == (0,) * 8


@pytest.mark.gpu
def test_timestep_without_caches_reuses_the_context_work_set_like_a_fresh_one(eu):
    """phiv_timestep! without caches keeps its work arrays and KrylovSubspace in the context between calls (allocation cost
    more than the call): a sequence of DIFFERENT calls on one context -- other inputs, horizons, tolerances, a larger m, more
    coefficient columns, a Hermitian operator -- must each equal the oracle, with the oracle's controller decisions."""
    rng = np.random.default_rng(21)
    n = 700
    A = c2_operator(n)
    As = c2_operator(n, sym=True)
    ctx = eu.Context()
    cases = [(A, 1, [1.0], 1e-6, None), (A, 1, [0.4, 2.5], 1e-9, None), (A, 3, [3.0], 1e-7, None), (As, 2, [1.5, 6.0], 1e-8, None),
             (A, 1, [2.0], 1e-7, 24), (A, 4, [0.7], 1e-6, None), (A, 1, [5.0], 1e-10, None)]
    for k, (M, ncoef, ts, tol, m) in enumerate(cases):
        B = rng.standard_normal((n, ncoef))
        kw = dict(adaptive=True, tol=tol)
        if m is not None:
            kw["m"] = m
        st, so = {}, {}
        U = eu.phiv_timestep(np.array(ts), eu.MIOperator(M, ctx), B, stats=st, **kw)
        Uo = ko.phiv_timestep(np.array(ts), M, B, stats=so, **kw)
        assert (st["num_timesteps"], st["matvecs"], st["m"]) == (so["num_timesteps"], so["matvecs"], so["m"]), (k, st, so)
        close(U, Uo, 1e-12, "cache-less phiv_timestep, call %d of a sequence on one context vs oracle" % k)


@pytest.mark.gpu
def test_recycled_krylov_subspace_is_indistinguishable_from_a_fresh_one(eu):
    """expv_mi_ks_destroy keeps the storage (context option "recycle") and the next create of the same shape takes it over:
    convenience calls that build a KrylovSubspace per call -- phiv(t, A, b, k), arnoldi(A, b) with changing inputs, a Lanczos
    run after an Arnoldi run, a happy breakdown in between -- give what a context with recycling off gives, bit for bit,
    and match the oracle."""
    rng = np.random.default_rng(5)
    n = 900
    A = c2_operator(n)
    As = c2_operator(n, sym=True)
    ctxs = [eu.Context(), eu.Context()]
    ctxs[1].set_option("recycle", 0)
    ops = [(eu.MIOperator(A, c), eu.MIOperator(As, c)) for c in ctxs]
    e1 = np.zeros(n); e1[0] = 1.0
    calls = [("phiv", 0, 0.7, 3, 20), ("phiv", 0, 1.3, 1, 20), ("phiv", 1, 0.5, 2, 20), ("H", 0, None, None, 20),
             ("phiv", 0, 2.0, 2, 20), ("H", 1, None, None, 20), ("phiv", 0, 0.3, 4, 12), ("phiv", 0, 0.9, 2, 20)]
    for k, (kind, which, t, kk, m) in enumerate(calls):
        b = rng.standard_normal(n)
        M = (A, As)[which]
        outs = []
        for c, (opA, opS) in zip(ctxs, ops):
            op = (opA, opS)[which]
            if kind == "phiv":
                outs.append(np.asarray(eu.phiv(t, op, b, kk, m=m)))
            else:
                Ks = eu.arnoldi(op, b, m=m)
                outs.append(np.array(Ks.getH()))
                del Ks
        assert np.array_equal(outs[0], outs[1]), "call %d: recycled and freshly allocated subspace differ" % k
        if kind == "phiv":
            close(outs[0], ko.phiv(t, M, b, kk, m=m), 1e-11, "phiv through a recycled KrylovSubspace, call %d vs oracle" % k)
        else:
            Ko = ko.arnoldi(M, b, m=m)
            close(outs[0], Ko.getH(), 1e-12, "H through a recycled KrylovSubspace, call %d vs oracle" % k)


@pytest.mark.gpu
def test_values_only_update_equals_a_new_operator(eu):
    """expv_mi_op_update_values: new values on an unchanged pattern refill every stored form on the device.  For each storage
    class -- banded DIA (the single-pass step), grid stencil (general DIA / wave form), regular rows (SELL only), irregular rows
    (plain CSR), complex, created from CSR and from CSC -- the updated operator must behave bit for bit like one built from the
    new matrix, and report its ishermitian / opnorm."""
    rng = np.random.default_rng(17)
    def perturb(A, herm=False):
        B = A.copy()
        B.data = B.data * (1.0 + 0.3 * rng.standard_normal(B.nnz))
        if herm:
            B = ((B + B.conj().T) * 0.5).asformat(A.format)
            B.sort_indices()
        return B
    n = 3000
    banded = c2_operator(n)
    gx = 50
    grid = (sp.kron(sp.eye(n // gx), sp.diags([1.0, -2.0, 1.0], [-1, 0, 1], shape=(gx, gx))) +
            sp.kron(sp.diags([0.7, -1.0, 0.9], [-1, 0, 1], shape=(n // gx, n // gx)), sp.eye(gx)))
    reg = sp.random(n, n, density=6.0 / n, random_state=3, format="csr") + sp.diags(np.full(n, -3.0))
    irr = sp.random(n, n, density=4.0 / n, random_state=4, format="lil")
    irr[7, :200] = 0.01
    irr = irr.tocsr() + sp.diags(np.full(n, -2.0))
    cases = [("banded csc", banded.tocsc(), False), ("banded csr", banded.tocsr(), False), ("banded symmetric pattern -> Hermitian", banded.tocsc(), True),
             ("grid stencil", grid.tocsc(), False), ("regular rows", reg.tocsc(), False), ("irregular rows", irr.tocsc(), False),
             ("complex banded", (banded * (1.0 + 0.2j)).tocsc(), False), ("complex -> Hermitian", (banded * (1.0 + 0.2j)).tocsc(), True)]
    ctx = eu.Context()
    for name, A0, herm in cases:
        A0.sort_indices()
        A1 = perturb(A0, herm)
        assert A1.nnz == A0.nnz and np.array_equal(A1.indices, A0.indices) and np.array_equal(A1.indptr, A0.indptr), name
        b = rng.standard_normal(n) + (1j * rng.standard_normal(n) if A0.dtype.kind == "c" else 0)
        op = eu.MIOperator(A0, ctx)
        w_before = np.asarray(eu.expv(0.4, op, b, m=20))
        op.update_values(A1)
        fresh = eu.MIOperator(A1, ctx)
        assert op.ishermitian == fresh.ishermitian == herm, (name, op.ishermitian, fresh.ishermitian)
        # (complex: |a| is a hypot on either side, device and host libm may differ in the last bit)
        assert abs(op.opnorm_inf - fresh.opnorm_inf) <= (0 if A0.dtype.kind != "c" else 1e-14 * fresh.opnorm_inf), (name, op.opnorm_inf, fresh.opnorm_inf)
        for kw in ({}, {"ishermitian": False}):
            w_upd = np.asarray(eu.expv(0.4, op, b, m=20, **kw))
            w_new = np.asarray(eu.expv(0.4, fresh, b, m=20, **kw))
            assert np.array_equal(w_upd, w_new), "%s: updated operator and new operator differ" % name
        assert not np.array_equal(w_upd, w_before), name
        close(w_upd, ko.expv(0.4, A1, b, m=20, ishermitian=False), 1e-12, "expv on a values-updated operator (%s) vs oracle" % name)
        y_upd, y_new = np.asarray(op.apply(b)) if hasattr(op, "apply") else None, np.asarray(fresh.apply(b)) if hasattr(fresh, "apply") else None
        if y_upd is not None:
            assert np.array_equal(y_upd, y_new), name
    # the convenience form: the same scipy object mutated in place between calls is refilled, not rebuilt
    A = banded.tocsc(); A.sort_indices()
    b = rng.standard_normal(n)
    eu.clear_operator_cache()
    w0 = np.asarray(eu.expv(0.4, A, b, m=20, ishermitian=False))
    A.data[:] = A.data * 1.5
    w1 = np.asarray(eu.expv(0.4, A, b, m=20, ishermitian=False))
    close(w1, ko.expv(0.4, A, b, m=20, ishermitian=False), 1e-12, "expv after an in-place change of A.data (convenience form) vs oracle")
    assert not np.array_equal(w0, w1)


@pytest.mark.gpu
def test_dense_operator_properties_do_not_depend_on_where_the_matrix_came_from(eu):
    """A dense operator handed over as a row-major numpy array (uploaded as it lies, laid out column-major on the device), as
    a column-major numpy array, or as a torch tensor already on the GPU reports the same opnorm(A, Inf) / ishermitian / nnz and
    applies identically -- in particular the library must not read a torch tensor (or the layout copy made for it) before
    torch has finished writing it."""
    import torch
    rng = np.random.default_rng(8)
    n = 3000
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    A[5, 7] = 0.0
    x = rng.standard_normal(n)
    ref = float(np.abs(A).sum(axis=1).max())
    for trial in range(3):
        ops = [eu.MIOperator(A), eu.MIOperator(np.asfortranarray(A)), eu.MIOperator(torch.as_tensor(A, device="cuda")),
               eu.MIOperator(torch.as_tensor(np.asfortranarray(A).T.copy(), device="cuda").t())]
        for op in ops:
            assert abs(op.opnorm_inf - ref) <= 4e-16 * ref * n ** 0.5, (trial, op.opnorm_inf, ref)
            assert op.opnorm_inf == ops[0].opnorm_inf and op.ishermitian == ops[0].ishermitian is False and op.nnz == n * n - 1
        ys = [np.asarray(eu.expv(0.3, op, x, m=12)) for op in ops]
        for y in ys[1:]:
            assert np.array_equal(y, ys[0]), trial
    S = A + A.T
    assert eu.MIOperator(torch.as_tensor(S, device="cuda")).ishermitian and eu.MIOperator(S).ishermitian


@pytest.mark.gpu
def test_ishermitian_of_sparse_operators_edge_cases(eu):
    """LinearAlgebra.ishermitian on a sparse matrix ignores stored zeros.  The creation-time test looks for one stored entry
    without its conjugate partner before it transposes anything, the update-time test runs on the device: both must agree
    with the dense definition on the awkward cases."""
    rng = np.random.default_rng(12)
    n = 6000
    def dense_herm(M):
        D = M.toarray()
        return bool(np.array_equal(D, D.conj().T))
    base = sp.random(n, n, density=5.0 / n, random_state=9, format="csr")
    H = (base + base.T).tocsr(); H.sort_indices()                       # Hermitian (real symmetric)
    late = H.copy().tolil(); late[5000, 17] = 0.25; late = late.tocsr(); late.sort_indices()   # one asymmetric entry far down
    zero_partner = H.copy().tolil(); zero_partner[40, 90] = 0.0; zero_partner[90, 40] = 0.0
    zero_partner = zero_partner.tocsr()
    stored_zero_only_one_side = H.copy().tolil(); stored_zero_only_one_side[7, 3000] = 1.0; stored_zero_only_one_side = stored_zero_only_one_side.tocsr()
    stored_zero_only_one_side[7, 3000] = 0.0                                  # explicit zero without a partner: still Hermitian
    Hc = (H + 1j * (sp.triu(H, 1) - sp.triu(H, 1).T)).tocsr(); Hc.sort_indices()   # complex Hermitian
    bad_diag = Hc.copy().tolil(); bad_diag[11, 11] = 1.0 + 0.5j; bad_diag = bad_diag.tocsr()   # diagonal not real
    cases = {"symmetric": H, "asymmetric entry in row 5000": late, "pair of stored zeros": zero_partner,
             "stored zero without partner": stored_zero_only_one_side, "complex Hermitian": Hc, "complex, diagonal not real": bad_diag,
             "plain non-symmetric": base.tocsr()}
    for name, M in cases.items():
        want = dense_herm(M)
        for fmt in ("csr", "csc"):
            Mf = M.asformat(fmt); Mf.sort_indices()
            op = eu.MIOperator(Mf)
            assert op.ishermitian == want, (name, fmt, op.ishermitian, want)
            op.update_values(Mf)                                             # the device-side test on the same values
            assert op.ishermitian == want, (name, fmt, "after update", op.ishermitian, want)
    # an update can make a non-Hermitian operator Hermitian and back
    A0 = H.copy(); A0.data = A0.data * (1.0 + 0.1 * rng.standard_normal(A0.nnz))
    op = eu.MIOperator(A0)
    assert not op.ishermitian
    assert op.update_values(H).ishermitian and not op.update_values(A0).ishermitian


@pytest.mark.gpu
def test_batch_pattern_cache_follows_a_changed_pattern(eu):
    """expv_batch keeps the DIA layout of the shared pattern (and its device permutation) in the context between calls.  Same
    n and nnz, other column indices; a pattern that comes back; values passed again on the cached pattern: every call equals
    the single-problem results."""
    rng = np.random.default_rng(33)
    n, nprob, m = 4000, 6, 20
    ctx = eu.Context()
    def pattern(offsets):
        M = sp.diags([rng.standard_normal(n - abs(o)) * 0.4 - (2.0 if o == 0 else 0.0) for o in offsets], offsets, format="csr")
        M.sort_indices()
        return M
    P1, P2 = pattern([-2, -1, 0, 1, 2]), pattern([-3, -1, 0, 1, 3])
    P3 = P1.copy()                                   # same n, same nnz, one entry elsewhere: (10, 12) -> (10, 5)
    k0 = P3.indptr[10]
    assert list(P3.indices[k0:k0 + 5]) == [8, 9, 10, 11, 12]
    P3.indices[k0:k0 + 5] = [5, 8, 9, 10, 11]
    assert P3.nnz == P1.nnz and P3.has_canonical_format
    for rnd, P in enumerate([P1, P2, P1, P3, P3, P1, P2]):
        vals = np.stack([P.data * (1.0 + 0.2 * rng.standard_normal(P.nnz)) for _ in range(nprob)])
        B = np.asfortranarray(rng.standard_normal((n, nprob)))
        W = eu.expv_batch(0.7, P, vals, B, m=m, ctx=ctx)
        for p in range(nprob):
            Ap = P.copy()
            Ap.data = vals[p].copy()
            close(W[:, p], ko.expv(0.7, Ap, B[:, p], m=m, ishermitian=False), 1e-12, "batch call %d, column %d vs oracle" % (rnd, p))


def test_handles_may_outlive_their_context_and_double_destroy_is_harmless(eu):
    """a host language may run finalizers in any order.  Destroying the context first leaves KrylovSubspace / operator
    / timestep-cache handles whose own destroy must free their memory without touching the dead context; destroying a
    KrylovSubspace twice (it became the context's recycled spare) is a no-op."""
    import ctypes as C
    from exponentialutilities_jl_amd import _lib as L
    lib = L.load()
    n = 4096
    A = c2_operator(n).tocsr()
    for order in ("ctx_first", "ctx_last"):
        ctx, ks, ks2, op, tsc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.expv_mi_ctx_create(0, None, C.byref(ctx)) == 0
        assert lib.expv_mi_ks_create(ctx, L.F64, L.F64, n, 10, 0, C.byref(ks)) == 0
        assert lib.expv_mi_ks_create(ctx, L.F64, L.F64, n, 12, 0, C.byref(ks2)) == 0
        ip, ix, va = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        assert lib.expv_mi_op_create_csr(ctx, L.F64, n, ip.ctypes.data, ix.ctypes.data, va.ctypes.data, 4, 0, C.byref(op)) == 0
        assert lib.expv_mi_timestep_caches_create(ctx, L.F64, n, 10, 1, C.byref(tsc)) == 0
        b = np.ones(n)
        o = L.ArnoldiOpts()
        lib.expv_mi_arnoldi_opts_default(C.byref(o))
        o.m = 10
        assert lib.expv_mi_arnoldi(ks, op, b.ctypes.data, L.HOST, C.byref(o)) == 0
        raw = C.c_void_p()
        assert lib.expv_mi_malloc(ctx, 1 << 20, C.byref(raw)) == 0      # (a host-language array: the Julia shim's MIVector)
        if order == "ctx_first":
            assert lib.expv_mi_ks_destroy(ks2) == 0          # becomes the context's spare ...
            assert lib.expv_mi_ks_destroy(ks2) == 0          # ... and a second destroy of it changes nothing
            assert lib.expv_mi_ctx_destroy(ctx) == 0         # frees the spare; ks / op / tsc are orphans now
            assert lib.expv_mi_ks_destroy(ks) == 0
            assert lib.expv_mi_op_destroy(op) == 0
            assert lib.expv_mi_timestep_caches_destroy(tsc) == 0
            assert lib.expv_mi_free(ctx, raw) == 0           # the array's finalizer after the context's: the dead handle is not read
        else:
            assert lib.expv_mi_free(ctx, raw) == 0
            assert lib.expv_mi_timestep_caches_destroy(tsc) == 0
            assert lib.expv_mi_op_destroy(op) == 0
            assert lib.expv_mi_ks_destroy(ks) == 0
            assert lib.expv_mi_ks_destroy(ks2) == 0
            assert lib.expv_mi_ctx_destroy(ctx) == 0
    # the library still works afterwards
    w = eu.expv(0.3, A, np.ones(n), m=10)
    close(w, ko.expv(0.3, A, np.ones(n), m=10), 1e-12, "expv after out-of-order handle destruction")


def test_c3_at_the_largest_single_gpu_size(eu):
    """BASELINE configs[2] at the largest size one MI355X holds: n = 163 840 dense fp64 (214.7 GB, generated on the device).
    No oracle can follow at this size, so the checks are size-independent: (i) mul! is linear to rounding, (ii) one entry of
    A x agrees with a dot product of that row taken by torch, (iii) the adaptive phiv_timestep driven by the dense operator
    and by the row-sharded operator at world size 1 (dist.RowShardedDense: library GEMV through the matrix-free callback) take
    the same controller decisions and give the same snapshot, (iv) the snapshot satisfies the defining ODE residual in the
    Krylov sense: the two runs at tol and tol/100 agree to ~tol."""
    import importlib.util, os, sys, torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if torch.cuda.get_device_properties(0).total_memory < 250e9:
        pytest.skip("needs a 288 GB device")
    sys.path.insert(0, root)
    import bench
    spec = importlib.util.spec_from_file_location("mi_dist", os.path.join(root, "exponentialutilities.jl_amd", "dist.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    n = 163_840
    ctx = eu.Context()
    A = bench.c3_rows(torch, torch.device("cuda", 0), n, 0, n)          # column-major n x n
    torch.cuda.synchronize()
    op = eu.MIOperator(A, ctx)
    assert op.shape == (n, n) and not op.ishermitian and op.nnz == n * n
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    y = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    torch.cuda.synchronize()
    ax, ay, axy = op @ x, op @ y, op @ (0.3 * x - 1.7 * y)
    ctx.sync()
    lin = float(torch.linalg.norm(axy - (0.3 * ax - 1.7 * ay)) / torch.linalg.norm(axy))
    close(lin, 0.0, 1e-13, "C3 n=163840: mul! linearity |A(ax+by) - aAx - bAy| / |.|", absolute=True)
    r = 98_765
    row = float(torch.dot(A[r, :].contiguous(), x))
    close(float(ax[r]), row, 1e-12 * float(torch.linalg.norm(A[r, :]) * torch.linalg.norm(x)), "C3 n=163840: (A x)[r] vs torch.dot of row r", absolute=True)
    B = torch.randn((5, n), dtype=torch.float64, device="cuda", generator=g).t()
    torch.cuda.synchronize()
    sd, ss, sf = {}, {}, {}
    Ud = eu.phiv_timestep(1.0, op, B, adaptive=True, tol=1e-7, m=10, stats=sd)
    sh = D.RowShardedDense(A, n)
    Us = eu.phiv_timestep(1.0, sh.operator(eu, ctx), B, adaptive=True, tol=1e-7, m=10, stats=ss)
    assert (sd["num_timesteps"], sd["matvecs"], sd["m"]) == (ss["num_timesteps"], ss["matvecs"], ss["m"]), (sd, ss)
    assert sh.applications >= ss["matvecs"]
    close(Us.cpu().numpy(), Ud.cpu().numpy(), 1e-12, "C3 n=163840: phiv_timestep, row-sharded (world 1) operator vs dense operator")
    Uf = eu.phiv_timestep(1.0, op, B, adaptive=True, tol=1e-9, m=10, stats=sf)
    close(Ud.cpu().numpy(), Uf.cpu().numpy(), 1e-6, "C3 n=163840: phiv_timestep at tol=1e-7 vs tol=1e-9 (bar 10 tol)")
    del op, A
    torch.cuda.empty_cache()


@pytest.mark.parametrize("T", [np.float32, np.complex64])
@pytest.mark.parametrize("n,m,iop", [(1000, 12, 0), (1025, 30, 0), (4100, 30, 3), (70_000, 30, 0), (70_001, 25, 0)])
def test_native_32bit_single_pass_step(eu, T, n, m, iop):
    """The single-pass step on 32-bit storage (tiles of 1024 / 512 rows: 4 / 2 rows per 16-byte pack, fp64 projection sums):
    banded operators in Float32 / ComplexF32 around the tile boundaries, full window, IOP and Lanczos, against the fp64 oracle
    on the same inputs at fp32 bars; the overlapped and the one-launch-after-the-other forms agree bit for bit."""
    cplx = np.dtype(T).kind == "c"
    rng = np.random.default_rng(n)
    d = [0.3 + 0.1 * rng.random(n - 2), 1.2 + 0.1 * rng.random(n - 1), -1.0 + 0.1 * rng.random(n), 0.8 + 0.1 * rng.random(n - 1),
         -0.1 + 0.1 * rng.random(n - 2)]
    A = sp.diags(d, [-2, -1, 0, 1, 2], format="csr")
    if cplx:
        A = (A * (1 + 0.25j)).tocsr()
    A = A.astype(T)
    b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)).astype(T)
    A64, b64 = A.astype(np.complex128 if cplx else np.float64), b.astype(np.complex128 if cplx else np.float64)
    ctx = eu.Context()
    op = eu.MIOperator(A, ctx)
    mm = min(m, 15) if cplx and iop == 0 else m                       # complex windows: <= 15 columns on the single-pass step
    w = eu.expv(0.6, op, b, m=mm, iop=iop, ishermitian=False)
    assert "pipeline" in eu.expv.last_stats["path"], eu.expv.last_stats
    assert np.asarray(w).dtype == np.dtype(T)
    close(np.asarray(w).astype(A64.dtype), ko.expv(0.6, A64, b64, m=mm, iop=iop, ishermitian=False), 2e-5,
          "expv single-pass %s n=%d m=%d iop=%d (fp32 bar)" % (np.dtype(T).name, n, mm, iop))
    Ks = eu.arnoldi(op, b, m=mm, iop=iop, ishermitian=False)
    Ko = ko.arnoldi(A64, b64, m=mm, iop=iop, ishermitian=False)
    close(Ks.getH().astype(A64.dtype), Ko.getH(), 3e-5, "arnoldi H single-pass %s n=%d m=%d iop=%d (fp32 bar)" % (np.dtype(T).name, n, mm, iop), mat=True)
    close(Ks.getV().astype(A64.dtype), Ko.getV(), 3e-5, "arnoldi V single-pass %s n=%d (max abs, fp32 bar)" % (np.dtype(T).name, n), absolute=True)
    ctx.set_pipeline_overlap(False)
    w2 = eu.expv(0.6, op, b, m=mm, iop=iop, ishermitian=False)
    ctx.set_pipeline_overlap(True)
    assert np.array_equal(np.asarray(w), np.asarray(w2))
    # Hermitian: Lanczos (window 2)
    S = ((A64 + A64.conj().T) * 0.5).astype(T).tocsr()
    ws = eu.expv(0.6, S, b, m=m)
    close(np.asarray(ws).astype(A64.dtype), ko.expv(0.6, S.astype(A64.dtype), b64, m=m), 2e-5,
          "expv Lanczos single-pass %s n=%d (fp32 bar)" % (np.dtype(T).name, n))


@pytest.mark.gpu
def test_two_processes_sharing_the_device_get_correct_results():
    """Two processes run overlapped factorisations on ONE GPU at the same time (ranks sharing a device, a second application):
    the residency the overlapped form relies on is then not guaranteed, its waits are bounded and a call whose wait expired is
    redone.  Every result must equal the one-launch-after-the-other result bit for bit, or to 1e-12 when the call was redone in
    another step form (tools/stress_shared_device.py; VERDICT r2, design / robustness)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_shared_device.py"), "6", "2"], cwd=root, capture_output=True,
                       text=True, timeout=600)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(rows) == 2, p.stdout + p.stderr
    for r in rows:
        assert r["mismatches"] == 0 and r["calls"] > 50 and r["worst_rel"] <= 1e-12, r


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128, 384, 1408])
def test_float32_columns_are_padded_to_whole_waves(eu, n):
    """Float32 moves 4 rows per lane, a wave 256: a basis column padded to 128 rows let the two-kernel step read the NEXT column
    through the tail of a wave whenever ceil(n / 128) is odd -- invisible on a fresh subspace (zeros), wrong (beta^2 off by the
    squared norm of the stale neighbour) from the second factorisation on.  Found by tests/fuzz_parity.py (seed 2026, case 2391:
    adaptive expv_timestep never terminated on the garbage error estimates).  Repeated factorisations on one subspace, growing
    and shrinking m, nine diagonals (two-kernel step), Lanczos and Arnoldi, then the adaptive time stepper."""
    rng = np.random.default_rng(7)
    offs = [-5, -4, -3, -2, 0, 2, 3, 4, 5]
    d = [rng.standard_normal(n - abs(o)) * 0.1 for o in offs]
    A = sp.diags(d, offs, shape=(n, n), format="csr")
    A = (((A + A.T) * 0.5) - 0.5 * sp.identity(n)).tocsr().astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    for herm in (True, False):
        Ks = eu.KrylovSubspace(np.float32, None, n, 5)
        for m in (5, 7, 5, 7, 3):
            eu.arnoldi_(Ks, A, b, m=m, ishermitian=herm)
            Ko = ko.arnoldi(A64, b64, m=m, ishermitian=herm)
            assert abs(Ks.beta - Ko.beta) <= 1e-5 * Ko.beta
            close(np.asarray(Ks.getH()).astype(np.float64), np.real(Ko.getH()), 2e-5,
                  "Float32 n=%d reused subspace, m=%d hermitian=%s: H (fp32 bar)" % (n, m, herm), mat=True)
    ts = np.array([0.66, 0.93])
    st = {}
    U = eu.expv_timestep(ts.copy(), A, b, tol=1e-5, m=5, adaptive=True, stats=st)
    Uo = ko.expv_timestep(ts.copy(), A64, b64, tol=1e-5, m=5, adaptive=True)
    close(np.asarray(U).astype(np.float64), Uo, 2e-4, "Float32 n=%d adaptive expv_timestep after reuse (fp32 bar)" % n)
    assert st["num_timesteps"] <= 4


@pytest.mark.gpu
def test_adaptive_controller_errors_like_the_reference_and_never_spins(eu):
    """krylov_phiv_adaptive.jl:470 takes ceil(Int, log(omega / gamma) / log(kappa)): when the error estimate does not move with m
    (an exhausted Krylov space: n = 5, m = 30) kappa is 1 and Julia throws InexactError.  The device driver used to carry on with
    an undefined integer and reject proposals for ever (found by tests/fuzz_parity.py, seed 81 case 3518); it now raises the same
    error, the oracle does too, and any sub-step is bounded by 1000 proposals."""
    rng = np.random.default_rng([81, 3518, 1])
    n = 5
    A0 = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n)
    A = 35.0 * ((A0 + A0.conj().T) * 0.5 - 0.5 * np.eye(n))
    B = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    ts = np.array([0.128, 0.148, 0.551])
    kw = dict(tol=1e-8, m=30, iop=7, adaptive=True)
    outcome = []
    for f in (lambda: eu.phiv_timestep(ts.copy(), A, B, **kw), lambda: ko.phiv_timestep(ts.copy(), A, B, **kw)):
        try:
            outcome.append(np.asarray(f()))
        except (ValueError, RuntimeError) as e:
            assert "InexactError" in str(e) or "did not reach the tolerance" in str(e), e
            outcome.append(None)
    assert (outcome[0] is None) == (outcome[1] is None), "device and oracle must fail (or succeed) together"
    if outcome[0] is not None:
        close(outcome[0], outcome[1], 1e-9, "phiv_timestep on an exhausted Krylov space")
    # and the engine is still usable afterwards
    b = rng.standard_normal(n) + 0j
    close(np.asarray(eu.expv(0.1, A, b, m=5)), ko.expv(0.1, A, b, m=5), 1e-10, "expv after a controller error")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float64, np.complex128, np.float32])
@pytest.mark.parametrize("kind", ["banded", "irregular", "dense"])
def test_error_estimate_mode_blocks_equal_the_step_by_step_form(eu, T, kind):
    """mode = :error_estimate (krylov_phiv_error_estimate.jl:149-207) runs its Lanczos steps in blocks through the ordinary
    factorisation (10, then 6 at a time, a true Lanczos continuation between blocks) and tests every step of a block on the host;
    the step-by-step form (context option ee_blocked = 0: 5 launches + an event per step) is the same recurrence one step at a
    time.  Same stopping step, same result, for stopping steps inside the first block, across block boundaries and at m."""
    from tests.test_gpu_parity import powerlaw_matrix
    cplx = np.dtype(T).kind == "c"
    single = np.dtype(T).itemsize == (8 if cplx else 4)
    rng = np.random.default_rng(17)
    n = 3000
    if kind == "banded":
        A = c2_operator(n, sym=True).astype(T)
    elif kind == "irregular":
        P = powerlaw_matrix(n, 5, cplx=cplx)
        A = ((P + P.conj().T) * 0.5).tocsr().astype(T)
    else:
        n = 600
        M = (rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)) / np.sqrt(n)
        A = ((M + M.conj().T) * 0.5 - 0.5 * np.eye(n)).astype(T)
    b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)).astype(T)
    ctx = eu.Context()
    op = eu.MIOperator(A, ctx)
    A64 = A.astype(np.complex128 if cplx else np.float64)
    b64 = b.astype(A64.dtype)
    seen = set()
    for m, rtol in ((30, 1e-2), (30, 1e-6), (30, 1e-10 if not single else 1e-5), (30, 1e-14), (7, 1e-14), (16, 1e-14), (17, 1e-14)):
        res = {}
        for blocked in (1, 0):
            ctx.set_option("ee_blocked", blocked)
            w = eu.expv(0.9, op, b, m=m, mode="error_estimate", rtol=rtol)
            res[blocked] = (int(eu.expv.last_subspace.m), np.asarray(w).astype(A64.dtype), np.asarray(eu.expv.last_subspace.getH()).astype(np.float64))
        assert res[1][0] == res[0][0], (m, rtol, res[1][0], res[0][0])
        seen.add(res[1][0])
        bar = 2e-5 if single else 1e-12
        close(res[1][1], res[0][1], bar, "error-estimate mode %s %s m=%d rtol=%g (stops at %d): blocks vs step by step" % (np.dtype(T).name, kind, m, rtol, res[1][0]))
        for kd in (0, -1):         # alpha and beta (what the mode defines; the super-diagonal is lanczos!'s own copy, arnoldi.jl:488)
            close(np.diag(res[1][2], kd), np.diag(res[0][2], kd), bar, "... H of the subspace, diagonal %d" % kd, mat=True)
        wo = ko.expv(0.9, A64, b64, m=m, mode="error_estimate", rtol=rtol)
        close(res[1][1], wo, 3e-4 if single else 1e-10, "... against the oracle")
    assert len(seen) >= 3, seen           # (the cases really stop at different steps)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["grid2d", "grid3d", "near_and_far"])
def test_float32_wave_form_on_general_diagonals(eu, shape):
    """Float32 operators made of a few diagonals with arbitrary offsets (structured-grid stencils) run the wave form of the single-pass
    step like their fp64 counterparts (tiles of 1024 rows, u_j gathered from its column in memory, offsets that are a multiple of
    the 4-row pack as one 16-byte load): path, H / w against the fp64 oracle at fp32 bars, overlapped = one launch after the other
    bit for bit, IOP window, sizes that are not a multiple of the tile."""
    rng = np.random.default_rng(23)
    if shape == "grid2d":
        k = 150
        n = k * k + 37
        offs = [-k, -1, 0, 1, k]
    elif shape == "grid3d":
        k = 28
        n = k ** 3
        offs = [-k * k, -k, -1, 0, 1, k, k * k]
    else:
        n = 40_000
        offs = [-9000, -8, -3, 0, 2, 4096, 12001]
    d = [(0.1 + 0.05 * rng.random(n - abs(o))) * (1 if o else -6.0) for o in offs]
    A = sp.diags(d, offs, shape=(n, n), format="csr").astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    ctx = eu.Context()
    ctx.set_option("patch", 0)                     # (the 2-D grid in its natural ordering: the patch form has its own tests)
    op = eu.MIOperator(A, ctx)
    for m, iop in ((20, 0), (31, 0), (25, 4)):
        ctx.set_pipeline_overlap(True)
        w = np.asarray(eu.expv(0.4, op, b, m=m, iop=iop, ishermitian=False)).copy()
        path = list(eu.expv.last_stats["path"])
        assert "pipeline" in path and "wave" in path, path
        ctx.set_pipeline_overlap(False)
        w2 = np.asarray(eu.expv(0.4, op, b, m=m, iop=iop, ishermitian=False)).copy()
        assert np.array_equal(w, w2), "overlapped and serial wave forms differ"
        assert w.dtype == np.float32
        close(w.astype(np.float64), ko.expv(0.4, A64, b64, m=m, iop=iop, ishermitian=False), 1e-5, "Float32 wave form %s m=%d iop=%d: expv (fp32 bar)" % (shape, m, iop))
    ctx.set_pipeline_overlap(True)
    # (H of a few steps: on this diagonally dominant operator fp32 rounding grows ~2.3x per column against an fp64 run)
    Ks = eu.arnoldi(op, b, m=6, ishermitian=False)
    Ko = ko.arnoldi(A64, b64, m=6, ishermitian=False)
    close(np.asarray(Ks.getH()).astype(np.float64), Ko.getH(), 2e-5, "Float32 wave form %s: H of 6 steps incl. H[7, 6] (fp32 bar)" % shape, mat=True)


@pytest.mark.gpu
def test_bench_line_contract():
    """`python bench.py --full` (short): ONE JSON line with the keys the driver reads -- metric / value / unit / n_gpus / steps /
    warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload, a `roofline` object for the
    dominant kernel (bound, achieved, peak, unit, frac, traffic) and a `cpu_baseline` object (value, unit, cores, kind, sample);
    value consistent with ms_per_step, fraction below 1."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the driver's command with --full, secondaries ON: the LAST stdout line is the record and must stay < 4 KB
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"],
                       cwd=root, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-2000:]
    out_lines = [l for l in p.stdout.splitlines() if l.strip()]
    last = out_lines[-1]
    assert len(last) < 4096, len(last)
    lines = [l for l in out_lines if l.startswith("{")]
    assert len(lines) == 1 and lines[0] is last, p.stdout[-2000:]
    d = json.loads(last)
    assert len(d["config"]["secondary_fracs"]) >= 30          # the flat {name: frac} map travels in the line ...
    for k in ("matrix_free_compiled", "c4_kiops_complex"):      # (round 6 keys)
        assert k in d["config"]["secondary_fracs"], k
    assert d["config"]["value_cold"] > 0 and d["config"]["ms_per_step_cold"] > 0
    full = json.load(open(os.path.join(root, "bench_full.json")))
    assert "secondary" in full and "kernels" in full["roofline"]          # ... the prose and the per-kernel tables in the side file
    # (BASELINE configs[2] at its largest single-GPU size needs 215 GB of the device: present when this process' parent holds little of it --
    #  the driver's stand-alone run --, an out-of-memory note instead when the test suite around it does)
    c3f = full["secondary"].get("c3_dense_phiv_timestep_n163840", {})
    assert ("frac" in c3f and "c3_dense_phiv_timestep_n163840" in d["config"]["secondary_fracs"]) or "out of memory" in c3f.get("error", ""), c3f
    assert full["value"] == pytest.approx(d["value"], rel=1e-8)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["dtype"] == "f64" and d["unit"] == "matvecs/s"
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and "workload" in d["config"]
    assert abs(d["value"] - 30 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0.3 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1


@pytest.mark.gpu
def test_bench_plain_run_times_the_headline_and_dumps_its_result(tmp_path):
    """A plain `python bench.py --gpus 1 --steps K --warmup W` times the headline alone (no cold pass, roofline, secondary entries or
    CPU baseline: those are --full) and prints one line with K timed steps; --dump-outputs DIR writes the w of the last timed step,
    which is the expv of the seeded problem."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["dtype"] == "f64" and d["unit"] == "matvecs/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 30 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert "roofline" not in d and "cpu_baseline" not in d and "secondary_fracs" not in d["config"]
    assert d["config"]["value_cold"] is None
    w = np.load(os.path.join(str(tmp_path), "w.npy"))
    assert w.dtype == np.float64 and w.shape == (1_000_000,)
    n = w.size
    wo, r = co.expv_csr(1.0, c2_operator(n), np.random.default_rng(3).standard_normal(n), m=30)
    assert r["m"] == 30
    close(w, wo, 1e-12, "bench.py --dump-outputs: w of the last timed step vs the C oracle (n = 1e6, m = 30)")


def _bench_under_launcher(extra, timeout=900):
    """bench.py as the driver launches it for N > 1 -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` -- with N = 1: backend nccl (= RCCL), a real process group, real
    collectives on the device, at world size 1 (the test box has one GPU)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1"] + extra,
                       cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_c5_under_the_launcher_runs_the_rccl_gather_at_world_size_1():
    """the RCCL code path (not gloo) has executed -- `bench.py --config c5 --gpus 1` as a subprocess under
    torch.distributed.run, backend nccl: process-group init, the all-reduce / all-gather of the rank checks, and THE collective of
    the path, all_gather_into_tensor of the result block on the device; the gathered matrix is then verified column by column
    against the single-problem entry point like at any world size."""
    d = _bench_under_launcher(["--config", "c5", "--nprob", "12", "--steps", "2", "--warmup", "1"])
    assert d["process_group"] == "nccl" and d["n_gpus"] == 1 and d["ranks_seen"] == 1 and len(d["devices"]) == 1
    assert d["gather"]["ms"] is not None and d["gather"]["ms"] > 0          # the final gather ran, alone, and was timed
    assert d["verified"]["max_rel_err"] <= 1e-12
    assert d["value"] > 0 and d["config"]["nprob"] == 12


@pytest.mark.gpu
def test_c3_under_the_launcher_runs_the_rccl_all_gather_per_application():
    """... and `--config c3 --gpus 1` the same way: the row-sharded dense operator performs its ONE all_gather_into_tensor per
    operator application over RCCL from inside the library's matrix-free callback (on the library's stream), at world size 1."""
    d = _bench_under_launcher(["--config", "c3", "--n3", "4096", "--steps", "2", "--warmup", "1"])
    assert d["process_group"] == "nccl" and d["ranks_seen"] == 1
    assert d["collectives_per_call"] >= d["applications_per_call"] > 0
    assert d["verified"]["replicas_bitwise_equal"] is True and d["config"]["n"] == 4096


@pytest.mark.gpu
def test_c2_under_the_launcher_at_world_size_1():
    """The headline config through the driver's N > 1 launch form at N = 1: barrier and per-rank gathers over RCCL around the timed
    region."""
    d = _bench_under_launcher(["--steps", "3", "--warmup", "1", "--no-secondary", "--no-cpu-baseline", "--no-serial-pass"])
    assert d["process_group"] == "nccl" and d["n_gpus"] == 1 and d["scaling"] == "weak" and d["value"] > 0
    assert len(d["per_rank_ms_per_step"]) == 1


@pytest.mark.gpu
def test_slow_progress_of_the_reference_controller_is_reported_not_changed(eu):
    """the reference's adaptive controller never lengthens a step that meets the tolerance
    (krylov_phiv_adaptive.jl:391-417), so a tiny seed step is kept for the whole interval.  The library reproduces that (same
    number of sub-steps as tend / tau) and says so: one notice per decade through the print callback -- a RuntimeWarning in the
    Python mirror, also without `verbose` -- and stats["stalled_steps"]."""
    import warnings
    n = 256
    A = c2_operator(n).tocsc()
    b = np.random.default_rng(2).standard_normal(n)
    st = {}
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        u = eu.expv_timestep(0.0125, A, b, tau=1e-6, adaptive=True, tol=1e-6, m=5, stats=st)
    assert st["num_timesteps"] >= 12_500 and st["stalled_steps"] >= 10_000, st
    msgs = [str(w.message) for w in rec if "without step growth" in str(w.message)]
    assert len(msgs) == 1 and "krylov_phiv_adaptive.jl:391-417" in msgs[0], msgs
    close(u, sl.expm(0.0125 * A.toarray()) @ b, 1e-9, "expv_timestep over 12 500 kept seed steps vs dense truth")
    st2 = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # an ordinary run: no notice, field zero
        eu.expv_timestep(1.0, A, b, adaptive=True, tol=1e-6, stats=st2)
    assert st2["stalled_steps"] == 0 and st2["num_timesteps"] < 100


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["nine_offsets_halo", "irregular_band_wave", "shuffled_grid_reordered"])
def test_float32_sell_slot_forms_of_the_single_pass_step(eu, shape):
    """the SELL-slot forms of the single-pass step in Float32 (4 rows per lane, slices of 256 rows, tiles of 1024):
    the halo form for a banded pattern that has no diagonal form (nine offsets with gaps), the wave form for columns within a band of
    the row without any diagonal structure, and an unstructured 2-D grid numbering that operator creation reorders onto the wave
    form.  Path, expv / H against the fp64 oracle at fp32 bars, overlapped = one launch after the other bit for bit, an IOP window,
    sizes off the tile boundaries."""
    rng = np.random.default_rng(29)
    want = ["pipeline"]
    if shape == "nine_offsets_halo":
        n = 70_003
        offs = [-8, -6, -5, -3, 0, 1, 2, 4, 7, -1]                       # 10 distinct offsets: no DIA form (> 8), bandwidth 8
        d = [(0.1 + 0.05 * rng.random(n - abs(o))) * (1 if o else -6.0) for o in offs]
        A = sp.diags(d, offs, shape=(n, n), format="csr")
    elif shape == "irregular_band_wave":
        n, band, k = 90_001, 1500, 5
        rows = np.repeat(np.arange(n), k)
        cols = np.clip(rows + rng.integers(-band, band + 1, size=n * k), 0, n - 1)
        A = sp.csr_matrix((rng.standard_normal(n * k) * 0.3, (rows, cols)), shape=(n, n))
        A.sum_duplicates()
        A = (A - 0.5 * sp.eye(n)).tocsr()                              # (a dominant diagonal makes y = A v ~ d v: MGS cancellation amplifies fp32 rounding per column)
        want.append("wave")
    else:
        k = 640
        n = k * k                                                      # 409 600 rows: 400 Float32 tiles -- the reach decides
        G = sp.diags([0.7, 1.1, -4.0, 0.9, 1.3], [-k, -1, 0, 1, k], shape=(n, n), format="csr")
        q = rng.permutation(n)
        A = G[q][:, q].tocsr()
        want.append("wave")
    A = A.astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    ctx = eu.Context()
    ctx.set_option("patch", 0)                 # (the Float32 SELL wave form behind reverse Cuthill-McKee; with patch = 1 the grid is cut into patches)
    op = eu.MIOperator(A, ctx)
    if shape == "shuffled_grid_reordered":
        assert op.reorder_info["reordered"] and op.reorder_info["bandwidth_after"] <= 2 * k, op.reorder_info
    for m, iop in ((12, 0), (31, 0), (20, 3)):
        if shape == "shuffled_grid_reordered" and m == 31:
            continue
        ctx.set_pipeline_overlap(True)
        w = np.asarray(eu.expv(0.3, op, b, m=m, iop=iop, ishermitian=False)).copy()
        path = list(eu.expv.last_stats["path"])
        assert all(p in path for p in want), (path, want)
        ctx.set_pipeline_overlap(False)
        w2 = np.asarray(eu.expv(0.3, op, b, m=m, iop=iop, ishermitian=False)).copy()
        assert np.array_equal(w, w2), "overlapped and serial forms differ"
        assert w.dtype == np.float32
        close(w.astype(np.float64), ko.expv(0.3, A64, b64, m=m, iop=iop, ishermitian=False), 2e-5,
              "Float32 SELL-slot form %s m=%d iop=%d: expv (fp32 bar)" % (shape, m, iop))
    ctx.set_pipeline_overlap(True)
    Ks = eu.arnoldi(op, b, m=6, ishermitian=False)
    Ko = ko.arnoldi(A64, b64, m=6, ishermitian=False)
    K32 = ko.arnoldi(A, b, m=6, ishermitian=False)                     # the oracle in Float32 arithmetic: the scale of the bar
    rH = close(K32.getH().astype(np.float64), Ko.getH(), 1e-3, "  the oracle in float32 arithmetic vs the fp64 oracle: H (%s)" % shape, mat=True)
    eH = close(np.asarray(Ks.getH()).astype(np.float64), Ko.getH(), max(2e-5, 20 * rH), "Float32 SELL-slot form %s: H of 6 steps incl. H[7, 6] (fp32 bar)" % shape, mat=True)
    close(np.asarray(Ks.getV()).astype(np.float64), Ko.getV(), max(2e-5, 20 * rH), "Float32 SELL-slot form %s: V (max abs, fp32 bar)" % shape, absolute=True)


def _fuzz_case_inputs(seed, index, call):
    """Inputs of one case of tests/fuzz_parity.py (its generator is deterministic in (seed, index)): the case is run through the
    harness with the device and oracle entry points replaced by recorders, so the test below sees exactly what the harness fed them."""
    import tests.fuzz_parity as fz
    rec = {}
    saved = (getattr(fz.eu, call), getattr(fz.ko, call))

    class _Captured(Exception):
        pass

    def cap_dev(*a, **kw):
        rec["dev"] = (a, dict(kw))
        raise ValueError("InexactError: captured")          # (a controller error: the harness goes on to the oracle side)

    def cap_ref(*a, **kw):
        rec["ref"] = (a, dict(kw))
        raise ValueError("InexactError: captured")
    setattr(fz.eu, call, cap_dev)
    setattr(fz.ko, call, cap_ref)
    try:
        fz.one_case(seed, index)
    finally:
        setattr(fz.eu, call, saved[0])
        setattr(fz.ko, call, saved[1])
    assert "dev" in rec and "ref" in rec, "fuzz case %d/%d is not a %s case any more (generator changed?)" % (seed, index, call)
    return rec


@pytest.mark.gpu
def test_fuzz_pin_amplifying_hermitian_operator_controller_paths(eu):
    """seed 2027 case 22242 of the randomised hunt -- a dense Hermitian ComplexF64 operator with eigenvalues up to
    +80, adaptive expv_timestep to t = 1.34: exp(tA) amplifies by ~1e45.  The harness classifies the run (device: controller error,
    oracle: a result) as "not a parity question"; pinned here.  (a) On a horizon where rounding has not yet reached the error
    estimates both controllers take the SAME path: equal sub-step counts, equal Krylov dimensions, U to 1e-10.  (b) On the full
    horizon the device's failure is the reference controller's own fixed point (krylov_phiv_adaptive.jl:455-481: the proposal
    tau_new equals tau, m does not move, omega stays above delta -- the reference loops there for ever, :390-423), reported after
    1000 identical proposals as an ArgumentError -- not a device fault, not a wrong result."""
    rec = _fuzz_case_inputs(2027, 22242, "expv_timestep")
    (ts, A, b), kw = rec["dev"]
    (ts_o, A_o, b_o), kw_o = rec["ref"]
    assert kw["adaptive"] and np.iscomplexobj(A_o)
    Ad = np.asarray(A_o.toarray() if hasattr(A_o, "toarray") else A_o)
    ev = np.linalg.eigvalsh(Ad)
    assert np.allclose(Ad, Ad.conj().T) and ev.max() > 40 and float(np.max(ts)) > 1.2      # the amplifying Hermitian case
    # (a) a horizon both controllers agree on
    t_small = np.array([0.1])
    sd, so = {}, {}
    U = np.asarray(eu.expv_timestep(t_small.copy(), A, b, **dict(kw, stats=sd)))
    Uo = np.asarray(ko.expv_timestep(t_small.copy(), A_o, b_o, **dict(kw_o, stats=so)))
    assert sd["num_timesteps"] == so["num_timesteps"] and sd["m"] == so["m"], (sd, so)
    close(U, Uo, 1e-10, "amplifying Hermitian operator, t = 0.1: device vs oracle on the same controller path")
    # (b) the full horizon: the device ends in the reference controller's fixed point and says so
    # (round 6: which of the two it is depends on the last bits of the host's small exponentials -- the ComplexF64 products of
    #  host_dense.h changed their summation order this round and the device now FINISHES this horizon like the oracle does.  Both
    #  outcomes are the reference controller's; pinned: it is one of the two, never a hang, never another error, and a finished run
    #  agrees with the oracle's in the dominant direction -- exp(tA) amplifies by 1e45 there, relative accuracy survives.)
    log = []
    try:
        Ufull = np.asarray(eu.expv_timestep(np.asarray(ts).copy(), A, b, **dict(kw, verbose=True, out=log.append)))
        raised = None
    except (ValueError, RuntimeError) as ex:
        raised = ex
    if raised is not None:
        msg = str(raised)
        assert "did not reach the tolerance in 1000 proposals" in msg, msg
        import re
        props = [ln for ln in log if "tau" in ln and "error estimate" in ln]
        assert len(props) >= 500, (len(props), log[-5:])
        tail = props[-400:]
        taus = {re.search(r"tau = ([-+0-9.eE]+)", ln).group(1) for ln in tail}
        ms = {re.search(r"m = (\d+)", ln).group(1) for ln in tail}
        assert len(taus) == 1 and len(ms) == 1, (sorted(taus)[:4], sorted(ms), tail[-3:])      # tau_new == tau, m_new == m: the fixed point
        print("[pin] full horizon: the reference controller's fixed point, reported as an ArgumentError")
    else:
        Uo_full = np.asarray(ko.expv_timestep(np.asarray(ts_o).copy(), A_o, b_o, **dict(kw_o)))
        assert np.all(np.isfinite(Ufull)) and Ufull.shape == Uo_full.shape
        close(Ufull, Uo_full, 1e-6, "amplifying Hermitian operator, full horizon: a finished run against the oracle's (amplification 1e45)")
        print("[pin] full horizon: finished like the oracle")
    # and the library is usable afterwards
    close(np.asarray(eu.expv(0.01, A, b, m=10)), ko.expv(0.01, A_o, b_o, m=10), 1e-10, "expv after the controller error")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_fuzz_pin_zero_start_vector_on_a_recycled_subspace(eu, T):
    """seed 31337 case 11086 -- arnoldi! with a ZERO starting vector on a subspace that holds an earlier
    factorisation.  firststep! zeroes H, finds beta == 0 and returns with V untouched (arnoldi.jl:230-250, :366): beta = 0 and
    H = 0 EXACTLY, Ks.m as the reference leaves it, expv! = 0 exactly (krylov_phiv.jl:206-210), and the basis columns 2.. still hold
    the previous call's vectors (column 1: those or the zero vector b itself) -- on the single-pass, the two-kernel and the modular path."""
    rng = np.random.default_rng(91)
    n, m = 3000, 12
    cplx = np.dtype(T).kind == "c"
    for kind in ("banded", "random", "dense"):
        if kind == "banded":
            A = c2_operator(n).astype(T)
        elif kind == "random":
            A = (sp.random(n, n, density=4.0 / n, random_state=5, format="csr") - 0.5 * sp.identity(n, format="csr")).astype(T)
        else:
            A = (rng.standard_normal((300, 300)) / np.sqrt(300)).astype(T)
        nn = A.shape[0]
        b = (rng.standard_normal(nn) + (1j * rng.standard_normal(nn) if cplx else 0)).astype(T)
        Ks = eu.KrylovSubspace(T, T, nn, m)
        eu.arnoldi_(Ks, A, b, m=m, ishermitian=False)
        V_before = np.asarray(Ks.getV()).copy()
        z = np.zeros(nn, dtype=T)
        eu.arnoldi_(Ks, A, z, m=m, ishermitian=False)
        Ko = ko.KrylovSubspace(T, T, nn, m)
        ko.arnoldi_(Ko, A, b, m=m, ishermitian=False)
        ko.arnoldi_(Ko, A, z, m=m, ishermitian=False)
        assert Ks.beta == 0.0 and Ko.beta == 0.0
        assert Ks.m == Ko.m and bool(Ks.wasbreakdown) == bool(Ko.wasbreakdown), (kind, Ks.m, Ko.m)
        assert not np.any(np.asarray(Ks.getH())), "%s: H of a zero start vector must be exactly zero" % kind
        w = np.asarray(eu.expv_(np.full(nn, 7.0, dtype=T), 0.3, Ks))
        assert not np.any(w), "%s: expv! of a zero start vector must be exactly zero" % kind
        # (the reference leaves V as it was -- formally uninitialised, arnoldi.jl:236-238; here the first pass stores u_1 = b = 0 in
        #  column 1 before it knows beta, and nothing else is written)
        V_after = np.asarray(Ks.getV())
        assert np.array_equal(V_after[:, 1:], V_before[:, 1:]), "%s: a zero start vector must leave columns 2.. of the stored basis untouched" % kind
        assert np.array_equal(V_after[:, 0], V_before[:, 0]) or not np.any(V_after[:, 0]), "%s: column 1 is the old v_1 or the zero vector" % kind
        # the whole-call form too
        assert not np.any(np.asarray(eu.expv(0.3, A, z, m=m, ishermitian=False)))


@pytest.mark.gpu
def test_fuzz_pin_exhausted_krylov_space_m_not_below_n(eu):
    """seed 5151 case 459 -- n = 3 Hermitian dense, m = 35 > n, adaptive phiv_timestep.  The Krylov space is
    exhausted after n steps; whether the residual that the error estimate is built from comes out as exactly 0 or as 1e-17 |A|
    decides between Julia's InexactError at ceil(Int, log(omega / gamma) / log(kappa)) (krylov_phiv_adaptive.jl:470; kappa = 1: the
    estimate does not move with m) and a finished run.  Both are the reference's behaviour; the harness accepts either for m >= n.
    Pinned: the device's outcome is ONE OF THE TWO -- that InexactError (status ArgumentError, the :470 site in its text), or a result
    that equals the dense truth -- and so is the oracle's; never a hang, never another error, never a wrong result."""
    rec = _fuzz_case_inputs(5151, 459, "phiv_timestep")
    (ts, A, B), kw = rec["dev"]
    (ts_o, A_o, B_o), kw_o = rec["ref"]
    Ad = np.asarray(A_o.toarray() if hasattr(A_o, "toarray") else A_o).astype(np.complex128)
    n = Ad.shape[0]
    assert n <= kw["m"] and kw["adaptive"], (n, kw)
    ts = np.sort(np.asarray(ts, dtype=float))
    Bd = np.asarray(B_o).astype(np.complex128)
    p = Bd.shape[1] - 1
    # dense truth: u(t) = sum_k t^k phi_k(tA) B[:, k]  (krylov_phiv_adaptive.jl:118-121) through the block-matrix identity
    truth = []
    for t in ts:
        phis = dense_phis(t * Ad, p)
        truth.append(sum((t ** k) * (phis[k] @ Bd[:, k]) for k in range(p + 1)))
    truth = np.stack(truth, axis=1)
    outcomes = []
    for name, f in (("device", lambda: eu.phiv_timestep(ts.copy(), A, B, **kw)), ("oracle", lambda: ko.phiv_timestep(ts.copy(), A_o, B_o, **kw_o))):
        try:
            U = np.asarray(f()).astype(np.complex128)
            close(U.reshape(truth.shape), truth, 1e-6 * max(1.0, kw["tol"] / 1e-8), "%s: exhausted Krylov space, finished run vs dense truth" % name)
            outcomes.append("result")
        except (ValueError, RuntimeError) as e:
            assert "InexactError" in str(e) and ("470" in str(e) or "ceil" in str(e)), (name, str(e))
            outcomes.append("InexactError")
    assert set(outcomes) <= {"result", "InexactError"}
    # exact exhaustion (a diagonal operator, a start vector in the span of three eigenvectors): both sides take the same branch
    D = np.diag([-1.0, -2.0, -3.0]).astype(np.complex128)
    Bx = np.ones((3, 2), dtype=np.complex128)
    res = []
    for f in (lambda: eu.phiv_timestep(np.array([0.5]), D, Bx, tol=1e-8, m=35, adaptive=True), lambda: ko.phiv_timestep(np.array([0.5]), D, Bx, tol=1e-8, m=35, adaptive=True)):
        try:
            res.append(np.asarray(f()))
        except (ValueError, RuntimeError) as e:
            assert "InexactError" in str(e), e
            res.append(None)
    assert (res[0] is None) == (res[1] is None), "exact exhaustion: device and oracle must take the same branch"
    if res[0] is not None:
        close(res[0], res[1], 1e-10, "exact exhaustion: device vs oracle")
