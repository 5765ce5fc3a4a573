"""Adjoint and transpose operators built on the device (expv_mi_op_create_adjoint / expv_mi_op_adjoint_refresh; MIOperator.adjoint,
.transpose, .H, .T, .refresh): the reference's expv(t, A', b).

The yardstick is the operator expv_mi_op_create_csr_loc makes, on the same context, of the sorted-row CSR arrays of A' / transpose(A)
(tests/adjoint_cases.py: adjoint_arrays, held against scipy in tests/test_adjoint_cpu.py): from the checked arrays on the two take
the same tail, so n, nnz, ishermitian, opnorm_inf, reorder / patch info, the path counters, matvec and arnoldi / expv / phiv are
compared for bit equality.  On integer-valued operators the adjoint identity is asserted without a tolerance."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import adjoint_cases as ac
from tests import bsr_cases as bc
from tests import coo_cases as cc
from tests import dia_cases as dc
from tests.limits import tile_rows
from tests.test_gpu_bsr_operator import bsr_op, same_everything
from tests.test_gpu_device_operator import DTYPES, PATTERNS, RawOp, make_pattern, sprand_gputests, to_torch_sparse
from tests.test_gpu_dia_operator import on_device

pytestmark = pytest.mark.gpu
CODE = {"float64": 0, "complex128": 1, "float32": 2, "complex64": 3}
TRANSPOSE, ADJOINT = 1, 2


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def csr_loc(eu, ctx, rp, ci, va):
    """the operator expv_mi_op_create_csr_loc makes of zero-based CSR arrays that were brought to the device"""
    arrs = [eu.DeviceArray.from_host(np.ascontiguousarray(rp, dtype=np.int32), ctx)]
    if len(ci):
        arrs += [eu.DeviceArray.from_host(np.ascontiguousarray(ci, dtype=np.int32), ctx), eu.DeviceArray.from_host(np.ascontiguousarray(va), ctx)]
    p = [a.ptr for a in arrs] + [None, None]
    h = C.c_void_p()
    eu.api._check(eu._lib.load().expv_mi_op_create_csr_loc(ctx._h, CODE[np.dtype(va.dtype).name], len(rp) - 1, len(ci), p[0], p[1], p[2], 4, 0, 1,
                                                           C.byref(h)), ctx._h)
    return RawOp(eu, ctx, h)


def twin(eu, ctx, A, how):
    """the definition: the CSR-born operator of the restatement's arrays of the sorted scipy matrix A"""
    A = A.tocsr()
    A.sort_indices()
    rp, ci, va, _ = ac.adjoint_arrays(A.indptr, A.indices, A.data, how == ADJOINT)
    return csr_loc(eu, ctx, rp, ci, va)


def made(op, how):
    return op.adjoint() if how == ADJOINT else op.transpose()


def exact(x):
    return np.array(x).astype(np.complex128)


# ------------------------------------------------------------------ 1. same operator, same bits
# every element type once per pattern as the adjoint, and every pattern once as the plain transpose of a complex operator
SAME = [(p, T, ADJOINT) for p in PATTERNS for T in DTYPES] + \
       [(p, (np.complex128, np.complex64)[i % 2], TRANSPOSE) for i, p in enumerate(PATTERNS)]


@pytest.mark.parametrize("pattern,T,how", SAME)
def test_adjoint_of_a_device_csr_operator_is_the_csr_born_twin_bit_for_bit(eu, torch, pattern, T, how):
    A = make_pattern(pattern, T)
    n = A.shape[0]
    ctx = eu.Context()
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    if pattern == "c2_permuted":
        assert parent.reorder_info["reordered"]
    if pattern == "grid":
        assert parent.patch_info["patch_form"]
    ref = twin(eu, ctx, A, how)
    op = made(parent, how)
    what = "%s %s how=%d" % (pattern, np.dtype(T).name, how)
    assert op.src is None and op.shape == (n, n) and op.nnz == A.nnz and op.dtype == np.dtype(T), what
    same_everything(eu, ctx, op, ref, T, what)
    info = op.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (n + 1 + A.nnz) and info["value_bytes_to_host"] == 0, info
    assert info["coo_entries"] == 0 and info["sort_passes"] == 0, info
    # opnorm(A', Inf) is the one-norm of A: the largest column sum of moduli, summed in fp64.  A sum of L non-negative terms, each a
    # rounded modulus in the element type's precision, against numpy's in another order: 2 (L + 2) eps relative (the bound of
    # test_ishermitian_and_opnorm_of_a_device_born_operator)
    col = np.asarray(abs(A.astype(np.complex128 if np.dtype(T).kind == "c" else np.float64)).sum(axis=0)).ravel()
    L = int(np.max(np.bincount(A.indices, minlength=n)))
    eps = float(np.finfo(np.float32 if T in (np.float32, np.complex64) else np.float64).eps)
    assert op.opnorm_inf == ref.opnorm_inf
    assert abs(op.opnorm_inf - col.max()) <= 2 * (L + 2) * eps * col.max(), (what, op.opnorm_inf, col.max())


# ------------------------------------------------------------------ 2. every birth
@pytest.mark.parametrize("T,how", [(np.float64, ADJOINT), (np.complex128, ADJOINT), (np.float32, TRANSPOSE), (np.complex64, TRANSPOSE)])
@pytest.mark.parametrize("birth", ["coo", "bsr", "dia", "host_csc", "host_csr"])
def test_every_birth_of_the_parent(eu, torch, birth, T, how):
    ctx = eu.Context()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
    if birth == "coo":          # shuffled triplets with repeats: summed at creation, duplicate-free once stored
        n = 200
        row, col, vals = cc.random_triplets(n, 900, T, seed=12, repeat_share=0.15, ends=True)
        parent = eu.MIOperator.from_coo(dev(row), dev(col), dev(vals), n, ctx=ctx)
        M = cc.expected_csr(row, col, vals, n)
        assert M.nnz < len(row) and parent.nnz == M.nnz
    elif birth == "bsr":
        ptr, idx, vals = bc.block_tridiagonal(40, 3, T)
        parent = bsr_op(eu, torch, ctx, ptr, idx, vals)
        M = bc.scalar_matrix(ptr, idx, vals, 3)
    elif birth == "dia":
        n, offs = 300, dc.scramble([-17, -1, 0, 1, 17])
        data = dc.pack(dc.random_diagonals(offs, n, T), offs, n, "col", T)
        parent = eu.MIOperator.from_dia(on_device(torch, data), offs, n, "col", ctx=ctx)
        M = dc.scalar_matrix(data, offs, n, "col")
    else:
        M = ac.upper(257, T)
        M = M.tocsc() if birth == "host_csc" else M
        parent = eu.MIOperator(M, ctx)
    M = sp.csr_matrix(M)
    M.sort_indices()
    assert parent.nnz == M.nnz
    same_everything(eu, ctx, made(parent, how), twin(eu, ctx, M, how), T, "%s %s how=%d" % (birth, np.dtype(T).name, how))


# ------------------------------------------------------------------ 3. the adjoint identity, exactly
# where slices and tiles begin and end, and one n just past two tiles of the widest single-pass step (the 4-byte element type's)
SIZES = [1, 2, 127, 128, 129, 513, 2 * tile_rows(4) + 1]


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_adjoint_identity_holds_exactly_on_integer_operators(eu, torch, n, T):
    ctx = eu.Context()
    x, y = ac.int_vector(n, T, 21), ac.int_vector(n, T, 22)
    for name in sorted(ac.CASES):
        S = ac.CASES[name](n, T)
        A = eu.MIOperator(to_torch_sparse(torch, S), ctx)
        AH, AT = A.adjoint(), A.transpose()
        Sx = S.astype(np.complex128)
        Ax, AHy, ATx = exact(A.matvec(x)), exact(AH.matvec(y)), exact(AT.matvec(x))
        # (every partial sum is an integer below n * 24 < 2^24: exact in every element type)
        assert np.array_equal(Ax, Sx @ exact(x)), (name, n)
        assert np.array_equal(AHy, Sx.conj().T @ exact(y)), (name, n)
        assert np.array_equal(ATx, Sx.T @ exact(x)), (name, n)
        assert np.vdot(exact(y), Ax) == np.vdot(AHy, exact(x)), (name, n)
        assert AH.nnz == S.nnz and AT.nnz == S.nnz, "stored zeros stay stored"


# ------------------------------------------------------------------ 4. involution
@pytest.mark.parametrize("pattern,T", [("sprand", np.complex128), ("c2_permuted", np.float64), ("powerlaw", np.complex64)])
def test_adjoint_of_the_adjoint_is_the_csr_born_operator(eu, torch, pattern, T):
    A = make_pattern(pattern, T)
    ctx = eu.Context()
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    same_everything(eu, ctx, parent.H.H, csr_loc(eu, ctx, A.indptr, A.indices, A.data), T, "%s: A'' vs A" % pattern)


@pytest.mark.parametrize("T", DTYPES)
def test_transpose_and_adjoint_compose_to_the_conjugate(eu, torch, T):
    n = 300
    ctx = eu.Context()
    S = ac.upper(n, T)
    A = eu.MIOperator(to_torch_sparse(torch, S), ctx)
    x = ac.int_vector(n, T, 5)
    want = S.astype(np.complex128).conj() @ exact(x)
    assert np.array_equal(exact(A.T.H.matvec(x)), want) and np.array_equal(exact(A.H.T.matvec(x)), want)
    if np.dtype(T).kind != "c":      # real element types: the two are the same operator
        same_everything(eu, ctx, A.H, A.T, T, "A' vs transpose(A), %s" % np.dtype(T).name)


# ------------------------------------------------------------------ 5. refresh
@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("pattern", ["c2", "c2_permuted", "sprand"])
def test_refresh_is_creating_the_adjoint_anew(eu, torch, pattern, T):
    A = make_pattern(pattern, T)
    symmetric_pattern = pattern != "sprand"
    if symmetric_pattern:      # Hermitian values on the same pattern
        A = (A + A.conj().T).tocsr().astype(T)
        A.sort_indices()
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    flipped = A.copy()
    flipped.data = np.where(A.indices > rows, -A.data, A.data)      # upper triangle negated: not Hermitian any more
    ctx = eu.Context()
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    adj = parent.adjoint()
    assert adj.ishermitian == symmetric_pattern and parent.ishermitian == symmetric_pattern
    for step, (M, herm) in enumerate(((flipped, False), (A, symmetric_pattern))):
        parent.update_values(torch.as_tensor(M.data).cuda())
        assert adj.refresh(parent) is adj
        assert adj.ishermitian == herm, (pattern, step)
        same_everything(eu, ctx, adj, parent.adjoint(), T, "%s %s refresh %d" % (pattern, np.dtype(T).name, step))
        same_everything(eu, ctx, adj, twin(eu, ctx, M, ADJOINT), T, "%s %s refresh %d vs twin" % (pattern, np.dtype(T).name, step), m=10)


def test_refresh_from_a_recreated_parent_and_refusals(eu, torch):
    T = np.complex128
    A = make_pattern("sprand", T)
    ctx = eu.Context()
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    adj = parent.adjoint()
    del parent                                  # the adjoint owns what it needs
    B = A.copy()
    B.data = B.data * (2.0 - 1.0j)
    again = eu.MIOperator(to_torch_sparse(torch, B), ctx)      # the same pattern, created anew
    adj.refresh(again)
    same_everything(eu, ctx, adj, twin(eu, ctx, B, ADJOINT), T, "refresh from a re-created parent")
    # another nnz, another element type, another context, not adjoint-born
    other = eu.MIOperator(to_torch_sparse(torch, sprand_gputests(1000, seed=9).astype(T)), ctx)
    assert other.nnz != adj.nnz
    with pytest.raises(eu.ExpvMIError, match="op_adjoint_refresh"):
        adj.refresh(other)
    with pytest.raises(eu.ExpvMIError, match="op_adjoint_refresh"):
        adj.refresh(eu.MIOperator(to_torch_sparse(torch, B.astype(np.complex64)), ctx))
    with pytest.raises(eu.ExpvMIError, match="op_adjoint_refresh"):
        adj.refresh(eu.MIOperator(to_torch_sparse(torch, B), eu.Context()))
    with pytest.raises(TypeError, match="adjoint"):
        again.refresh(adj)
    lib = eu._lib.load()
    assert lib.expv_mi_op_adjoint_refresh(again._h, adj._h) == 2
    # astype and the matrix forms of update_values point to the parent
    with pytest.raises(TypeError, match=r"parent\.astype"):
        eu.MIOperator(to_torch_sparse(torch, A.real.astype(np.float64).tocsr()), ctx).adjoint().astype(np.complex128)
    with pytest.raises(TypeError, match="refresh"):
        adj.update_values(B)
    with pytest.raises(TypeError, match="refresh"):
        adj.update_values(to_torch_sparse(torch, B))
    # bare values in the adjoint's own sorted-row order are the ordinary value update
    rp, ci, va, _ = ac.adjoint_arrays(A.indptr, A.indices, A.data, True)
    adj.update_values(va)
    same_everything(eu, ctx, adj, twin(eu, ctx, A, ADJOINT), T, "update_values in the adjoint's order")


@pytest.mark.parametrize("async_outputs", [False, True])
def test_back_to_back_refreshes_reproduce_their_bits(eu, torch, async_outputs):
    T = np.float64
    A = make_pattern("c2_permuted", T)
    ctx = eu.Context(async_outputs=async_outputs)
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    adj, fresh = parent.transpose(), parent.transpose()
    x = np.random.default_rng(8).standard_normal(A.shape[0])
    y0 = np.array(fresh.matvec(x))
    for _ in range(3):
        adj.refresh(parent)
        assert np.array_equal(np.array(adj.matvec(x)), y0) and adj.opnorm_inf == fresh.opnorm_inf
    assert np.array_equal(np.array(eu.expv(0.3, adj, x, m=20)), np.array(eu.expv(0.3, fresh, x, m=20)))


# ------------------------------------------------------------------ 6. dense
def padded_parent(torch, n, T, pad):
    """(buf, view): an n x n column-major device view with leading dimension n + pad whose padding rows hold NaN"""
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if np.dtype(T).kind == "c" else 0)
    buf = torch.full((n, n + pad), float("nan"), dtype=torch.as_tensor(np.zeros(1, dtype=T)).dtype, device="cuda")
    view = buf.t()[:n, :]                       # element (i, j) at j (n + pad) + i
    view.copy_(torch.as_tensor(a.astype(T)))
    return buf, view


DENSE = [(1, np.float64, 3), (1, np.complex64, 3), (31, np.complex128, 3), (31, np.float32, 3), (32, np.float32, 4), (32, np.complex128, 1),
         (33, np.complex64, 3), (33, np.float64, 2), (65, np.float64, 3), (65, np.complex128, 5), (257, np.complex64, 3), (257, np.float32, 3)]


@pytest.mark.parametrize("n,T,pad", DENSE)
def test_dense_adjoint_is_an_owned_packed_copy(eu, torch, n, T, pad):
    buf, view = padded_parent(torch, n, T, pad)
    before = buf.cpu().numpy().tobytes()
    ctx = eu.Context()
    parent = eu.MIOperator(view, ctx)
    x = np.random.default_rng(1).standard_normal(n).astype(T)
    for how in (ADJOINT, TRANSPOSE):
        op = made(parent, how)
        packed = (torch.conj_physical(view) if how == ADJOINT else view).contiguous().t()      # column-major, leading dimension n
        assert n == 1 or (packed.stride(0), packed.stride(1)) == (1, n)
        ref = eu.MIOperator(packed, ctx)
        what = "dense n=%d %s how=%d" % (n, np.dtype(T).name, how)
        assert np.isfinite(op.opnorm_inf), what + ": padding was read"
        same_everything(eu, ctx, op, ref, T, what)
    assert buf.cpu().numpy().tobytes() == before, "the parent tensor and its padding are unchanged"
    y0 = np.array(op.matvec(x))
    view.zero_()
    torch.cuda.synchronize()
    assert np.array_equal(np.array(op.matvec(x)), y0), "the adjoint owns a copy"
    op.refresh(parent)
    assert op.opnorm_inf == 0.0 and op.nnz == 0 and np.array_equal(np.array(op.matvec(x)), np.zeros(n, dtype=T))


# ------------------------------------------------------------------ 7. refusals and corners
def test_matrix_free_operator_has_no_adjoint(eu, torch):
    op = eu.MIOperator(None, matvec=lambda x: 2 * x, shape=(16, 16), dtype=np.float64)
    with pytest.raises(eu.ExpvMIError, match="op_create_adjoint") as e:
        op.adjoint()
    assert e.value.kind == "Unsupported"
    with pytest.raises(eu.ExpvMIError, match="how must be"):
        eu.MIOperator(ac.band(8, np.float64))._adjoint(3)


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_empty_operators(eu, torch, T):
    ctx = eu.Context()
    z = eu.MIOperator(sp.csr_matrix((5, 5), dtype=T), ctx).adjoint()
    assert z.shape == (5, 5) and z.nnz == 0 and z.opnorm_inf == 0.0
    assert np.array_equal(np.array(z.matvec(np.arange(1, 6).astype(T))), np.zeros(5, dtype=T))
    z.refresh(eu.MIOperator(sp.csr_matrix((5, 5), dtype=T), ctx))
    e = eu.MIOperator(sp.csr_matrix((0, 0), dtype=T), ctx).transpose()
    assert e.shape == (0, 0) and e.nnz == 0
    assert np.array(e.matvec(np.zeros(0, dtype=T))).shape == (0,)


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_unsorted_rows_with_a_repeated_coordinate(eu, torch, T):
    n = 400
    S = ac.upper(n, T)
    ip, ix, va = ac.with_repeat(S)
    At = torch.sparse_csr_tensor(torch.as_tensor(ip), torch.as_tensor(ix), torch.as_tensor(va), size=S.shape).cuda()
    ctx = eu.Context()
    parent = eu.MIOperator(At, ctx)
    assert parent.nnz == S.nnz + 1
    x = ac.int_vector(n, T, 3)
    for how in (ADJOINT, TRANSPOSE):
        op = made(parent, how)
        assert op.nnz == parent.nnz, "the repeats stay separate entries"
        Sx = S.astype(np.complex128)
        assert np.array_equal(exact(op.matvec(x)), (Sx.conj().T if how == ADJOINT else Sx.T) @ exact(x))
        again = made(parent, how)      # deterministic: a second creation gives the same operator
        same_everything(eu, ctx, op, again, T, "repeat, how=%d" % how)


def test_second_adjoint_of_a_pattern_takes_its_plan_from_the_cache(eu, torch):
    from tests._util import c2_operator
    from tests.test_gpu_parity import _shuffle
    A = _shuffle(c2_operator(30_000), 23)
    A.sort_indices()
    ctx = eu.Context()
    parent = eu.MIOperator(to_torch_sparse(torch, A), ctx)
    eu.plan_cache(clear=True)                   # (the pattern is symmetric: the parent's plan would serve the adjoint too)
    first = parent.adjoint()
    second = parent.adjoint()
    assert first.reorder_info["reordered"] and not first.ingest_info["plan_cached"]
    assert second.ingest_info["plan_cached"]
    same_everything(eu, ctx, second, first, np.float64, "plan from the cache")


def test_reference_gpu_test_shape_with_the_adjoint(eu, torch):
    """test/gpu/gputests.jl:41-58 with A' in the operator's place: expv, expv_timestep and the Taylor entry"""
    T = np.complex128
    A = sprand_gputests(1000)
    ctx = eu.Context()
    AH = eu.MIOperator(to_torch_sparse(torch, A), ctx).H
    ref = twin(eu, ctx, A, ADJOINT)
    b = np.random.default_rng(6).standard_normal(1000) + 0j
    ts = np.array([0.05, 0.1])
    assert np.array_equal(np.array(eu.expv(0.1, AH, b)), np.array(eu.expv(0.1, ref, b)))
    assert np.array_equal(np.array(eu.expv_timestep(ts, AH, b)), np.array(eu.expv_timestep(ts, ref, b)))
    assert np.array_equal(np.array(eu.expv_taylor(0.1, AH, b)), np.array(eu.expv_taylor(0.1, ref, b)))
