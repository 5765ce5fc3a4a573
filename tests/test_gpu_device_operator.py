"""Sparse operators created from CSR / CSC arrays that live on the device (expv_mi_op_create_csr_loc / _csc_loc, MIOperator of a
torch.sparse_csr / torch.sparse_csc tensor): test/gpu/gputests.jl:41-58 hands expv / expv_timestep a CuSparseMatrixCSR.

The yardstick is the operator created from the same matrix on the host.  Both run the same planners on the same pattern and fill
the same stored forms from the same values, so everything that does not depend on HOW the value-dependent properties were
evaluated is compared for bit equality (m and opnorm= are given explicitly); opnorm(A, Inf) itself has a derived bound."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_oracle as ko
from tests._util import c2_operator, close, stencil2d
from tests.test_gpu_parity import TOL, _shuffle, powerlaw_matrix

pytestmark = pytest.mark.gpu
ARGUMENT_ERROR = 2          # EXPV_MI_ARGUMENT_ERROR


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def sprand_gputests(n, seed=0x0451, per_row=10):
    """the matrix of test/gpu/gputests.jl:41-43: sprand(ComplexF64), upper triangle + a little noise anywhere"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=per_row / n, random_state=rng, dtype=np.float64) \
        + 1j * sp.random(n, n, density=per_row / n, random_state=rng, dtype=np.float64)
    A = (sp.triu(A, 1) + sp.random(n, n, density=1 / n, random_state=rng) * (1 + 1j)).tocsr()
    A.sort_indices()
    return A


def make_pattern(pattern, T):
    cplx = np.dtype(T).kind == "c"
    if pattern == "c2":
        A = c2_operator(20_000)
    elif pattern == "grid":
        A = stencil2d(128)
    elif pattern == "c2_permuted":
        A = _shuffle(c2_operator(20_000), 11)
    elif pattern == "sprand":
        A = sprand_gputests(1000)
    else:
        A = powerlaw_matrix(6000, 77, cplx=cplx)
    A = A.tocsr()
    if not cplx and np.iscomplexobj(A):
        A = A.real.tocsr()
    A = A.astype(np.complex128 if cplx else np.float64)
    if cplx and pattern not in ("sprand", "powerlaw"):      # give the real test operators an imaginary part
        A.data = A.data * (1.0 + 0.25j * np.cos(np.arange(A.nnz)))
    A = A.astype(T)
    A.sort_indices()
    return A


def to_torch_sparse(torch, A, idx=np.int32, fmt="csr", device="cuda"):
    A = A.tocsr() if fmt == "csr" else A.tocsc()
    mk = torch.sparse_csr_tensor if fmt == "csr" else torch.sparse_csc_tensor
    return mk(torch.as_tensor(A.indptr.astype(idx)), torch.as_tensor(A.indices.astype(idx)), torch.as_tensor(A.data.copy()),
              size=A.shape).to(device)


def infos(op):
    r, p = dict(op.reorder_info), dict(op.patch_info)
    r.pop("setup_s")
    return r, p


def run_all(eu, ctx, op, b, m, opnorm):
    """the products compared for bit equality + the step form they ran"""
    c0 = ctx.counters()
    Ks = eu.arnoldi(op, b, m=m, ishermitian=False, opnorm=opnorm)
    H = np.array(Ks.getH())
    w = np.array(eu.expv(0.7, op, b, m=m, ishermitian=False, opnorm=opnorm))
    path = tuple(eu.expv.last_stats["path"])
    W = np.array(eu.phiv(0.5, op, b, 2, m=20, ishermitian=False, opnorm=opnorm))
    c1 = ctx.counters()
    return H, w, W, path, {k: c1[k] - c0[k] for k in c1}


def assert_same_operator(eu, ctx, opd, oph, T, what, m=25):
    assert opd.nnz == oph.nnz and opd.shape == oph.shape and opd.dtype == oph.dtype
    assert opd.ishermitian == oph.ishermitian, what
    assert infos(opd) == infos(oph), (what, infos(opd), infos(oph))
    n = oph.shape[0]
    rng = np.random.default_rng(3)
    b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(T).kind == "c" else 0)).astype(T)
    opn = float(oph.opnorm_inf)
    rd, rh = run_all(eu, ctx, opd, b, m, opn), run_all(eu, ctx, oph, b, m, opn)
    assert rd[3] == rh[3] and rd[4] == rh[4], (what, rd[3:], rh[3:])
    for name, x, y in zip(("arnoldi H", "expv", "phiv"), rd[:3], rh[:3]):
        assert np.all(np.isfinite(x)), (what, name)
        assert np.array_equal(x, y), "%s: %s of the device-born operator differs from the host-born one (max |d| %.3e)" % (
            what, name, float(np.max(np.abs(x - y))))


PATTERNS = ["c2", "grid", "c2_permuted", "sprand", "powerlaw"]
DTYPES = [np.float64, np.complex128, np.float32, np.complex64]


# ------------------------------------------------------------------ 1. same operator, same bits
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_device_csr_tensor_gives_the_host_born_operator_bit_for_bit(eu, torch, pattern, T, idx):
    A = make_pattern(pattern, T)
    ctx = eu.Context()
    oph = eu.MIOperator(A, ctx)
    opd = eu.MIOperator(to_torch_sparse(torch, A, idx), ctx)
    if pattern == "grid":
        assert oph.patch_info["patch_form"] and opd.patch_info["patch_form"]
    if pattern == "c2_permuted":
        assert oph.reorder_info["reordered"] and opd.reorder_info["reordered"]
    if pattern == "powerlaw":
        assert "overflow" in eu.host_pattern_info(A, T)["path"]
    assert_same_operator(eu, ctx, opd, oph, T, "%s %s %s" % (pattern, np.dtype(T).name, np.dtype(idx).name))
    # 7. what crossed to the host: the pattern, once; no values
    info = opd.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (A.shape[0] + 1 + A.nnz) and info["value_bytes_to_host"] == 0, info
    hi = oph.ingest_info
    assert not hi["from_device"] and hi["pattern_bytes_to_host"] == 0 and hi["value_bytes_to_host"] == 0, hi


# ------------------------------------------------------------------ 2. properties
@pytest.mark.parametrize("T", [np.float64, np.complex128, np.float32, np.complex64])
def test_ishermitian_and_opnorm_of_a_device_born_operator(eu, torch, T):
    cplx = np.dtype(T).kind == "c"
    n = 3000
    rng = np.random.default_rng(17)
    R = sp.random(n, n, density=8 / n, random_state=rng, dtype=np.float64)
    if cplx:
        R = R + 1j * sp.random(n, n, density=8 / n, random_state=rng, dtype=np.float64)
    Hm = (R + R.conj().T + sp.diags([rng.standard_normal(n)], [0])).tocsr().astype(T)      # Hermitian
    Hm.sort_indices()
    G = (Hm + sp.triu(R, 1).astype(T)).tocsr()                                             # not Hermitian
    G.sort_indices()
    # Hermitian, with explicit stored zeros at positions that have no partner
    free = sorted({(int(i), int(j)) for i, j in zip(rng.integers(0, n, 200), rng.integers(0, n, 200))
                   if i != j and Hm[i, j] == 0 and Hm[j, i] == 0})[:40]
    free = [(i, j) for i, j in free if (j, i) not in free]
    assert len(free) >= 10
    Zc = Hm.tocoo()
    rows = np.concatenate([Zc.row, [i for i, _ in free]])
    cols = np.concatenate([Zc.col, [j for _, j in free]])
    vals = np.concatenate([Zc.data, np.zeros(len(free), dtype=T)])
    Z = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    Z.sort_indices()
    assert Z.nnz == Hm.nnz + len(free)
    ctx = eu.Context()
    eps = float(np.finfo(np.float32 if T in (np.float32, np.complex64) else np.float64).eps)
    for name, M, herm in (("hermitian", Hm, True), ("general", G, False), ("hermitian + stored zeros", Z, True)):
        oph = eu.MIOperator(M, ctx)
        opd = eu.MIOperator(to_torch_sparse(torch, M), ctx)
        assert oph.ishermitian == herm and opd.ishermitian == herm, (name, oph.ishermitian, opd.ishermitian)
        # opnorm: a sum of L non-negative terms, each a rounded modulus, in two evaluation orders: 2 (L + 2) eps relative
        L = int(np.max(np.diff(M.indptr)))
        rel = abs(opd.opnorm_inf - oph.opnorm_inf) / oph.opnorm_inf
        print("[opnorm] %-28s %-10s device %.17g host %.17g rel %.3e (bound %.3e)" % (name, np.dtype(T).name, opd.opnorm_inf, oph.opnorm_inf, rel, 2 * (L + 2) * eps))
        assert rel <= 2 * (L + 2) * eps, (name, rel)
        oph.update_values(M)        # the same kernel now: equal, exactly
        assert oph.opnorm_inf == opd.opnorm_inf and oph.ishermitian == herm, (name, oph.opnorm_inf, opd.opnorm_inf)


# ------------------------------------------------------------------ 3. CSC
@pytest.mark.parametrize("T", [np.float64, np.complex128])
@pytest.mark.parametrize("pattern", ["c2", "c2_permuted", "sprand"])
def test_device_csc_tensor_gives_the_host_born_operator(eu, torch, pattern, T):
    A = make_pattern(pattern, T).tocsc()
    A.sort_indices()
    ctx = eu.Context()
    oph = eu.MIOperator(A, ctx)
    opd = eu.MIOperator(to_torch_sparse(torch, A, np.int64, "csc"), ctx)
    assert_same_operator(eu, ctx, opd, oph, T, "csc %s %s" % (pattern, np.dtype(T).name))
    info = opd.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (A.shape[0] + 1 + A.nnz) and info["value_bytes_to_host"] == 0, info


# ------------------------------------------------------------------ 4. 1-based int32 through the C ABI (Julia's layout)
class RawOp:
    """an operator handle made by a direct call, dressed as an MIOperator for the front ends"""

    def __new__(cls, eu, ctx, h):
        op = object.__new__(eu.MIOperator)
        lib = eu._lib.load()
        import weakref
        op.ctx, op.src, op._cb, op._h = ctx, None, None, h
        op._finalizer = weakref.finalize(op, lib.expv_mi_op_destroy, h)
        n_, nnz, herm, opn, dtc = C.c_int64(), C.c_int64(), C.c_int(), C.c_double(), C.c_int()
        assert lib.expv_mi_op_info(h, C.byref(n_), C.byref(nnz), C.byref(herm), C.byref(opn), C.byref(dtc)) == 0
        op.shape, op.nnz, op.ishermitian, op.opnorm_inf = (int(n_.value),) * 2, int(nnz.value), bool(herm.value), float(opn.value)
        op.dtype = op.src_dtype = np.dtype({0: np.float64, 1: np.complex128, 2: np.float32, 3: np.complex64}[dtc.value])
        return op


def raw_create(eu, ctx, fmt, A, idx, base, loc, nnz=None, idx_bytes=None, keep=None):
    lib = eu._lib.load()
    M = A.tocsr() if fmt == "csr" else A.tocsc()
    M.sort_indices()
    ptr, ind, val = (M.indptr + base).astype(idx), (M.indices + base).astype(idx), np.ascontiguousarray(M.data)
    code = {"float64": 0, "complex128": 1, "float32": 2, "complex64": 3}[M.dtype.name]
    if loc == 1:
        arrs = [eu.DeviceArray.from_host(x, ctx) for x in (ptr, ind, val)]
        ptrs = [a.ptr for a in arrs]
    else:
        arrs = [ptr, ind, val]
        ptrs = [a.ctypes.data for a in arrs]
    if keep is not None:
        keep.extend(arrs)
    h = C.c_void_p()
    fn = lib.expv_mi_op_create_csr_loc if fmt == "csr" else lib.expv_mi_op_create_csc_loc
    rc = fn(ctx._h, code, M.shape[0], M.nnz if nnz is None else nnz, ptrs[0], ptrs[1], ptrs[2],
            np.dtype(idx).itemsize if idx_bytes is None else idx_bytes, base, loc, C.byref(h))
    eu._lib.check(rc, ctx._h)
    return RawOp(eu, ctx, h)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_one_based_int32_device_arrays_through_the_c_abi(eu, fmt, T):
    ctx = eu.Context()
    for pattern in ("c2", "sprand"):
        A = make_pattern(pattern, T)
        oph = eu.MIOperator(A.tocsr() if fmt == "csr" else A.tocsc(), ctx)                # the old creators
        opd = raw_create(eu, ctx, fmt, A, np.int32, 1, 1)                                     # device arrays, Julia's layout
        oph2 = raw_create(eu, ctx, fmt, A, np.int32, 1, 0)                                    # loc = HOST through the new entry points
        assert_same_operator(eu, ctx, opd, oph, T, "1-based int32 device %s %s" % (fmt, pattern))
        assert_same_operator(eu, ctx, oph2, oph, T, "1-based int32 host via _loc %s %s" % (fmt, pattern))
        assert oph2.opnorm_inf == oph.opnorm_inf
        out = (C.c_int64 * 8)()
        assert eu._lib.load().expv_mi_op_ingest_info(oph2._h, out) == 0 and list(out) == [0] * 8
        assert eu._lib.load().expv_mi_op_ingest_info(opd._h, out) == 0 and out[0] == 1 and out[1] == 4 * (A.shape[0] + 1 + A.nnz) and out[2] == 0


# ------------------------------------------------------------------ 5. values refreshed on the device
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("pattern", ["c2", "c2_permuted", "powerlaw"])
def test_update_values_with_device_tensors_equals_creating_anew(eu, torch, fmt, pattern):
    T = np.float64
    A = make_pattern(pattern, T)
    A = A.tocsr() if fmt == "csr" else A.tocsc()
    A.sort_indices()
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.3 * np.cos(np.arange(A.nnz)))
    ctx = eu.Context()
    op = eu.MIOperator(to_torch_sparse(torch, A, np.int32, fmt), ctx)
    fresh = eu.MIOperator(to_torch_sparse(torch, A2, np.int32, fmt), ctx)
    assert op.reorder_info["reordered"] == (pattern == "c2_permuted")
    op.update_values(torch.as_tensor(A2.data.copy()).cuda())                  # bare values, the caller's entry order
    assert op.opnorm_inf == fresh.opnorm_inf and op.ishermitian == fresh.ishermitian
    assert_same_operator(eu, ctx, op, fresh, T, "update_values(values) %s %s" % (fmt, pattern))
    op.update_values(to_torch_sparse(torch, A, np.int32, fmt))                # a sparse tensor of the same layout: back to A
    first = eu.MIOperator(A, ctx)
    assert_same_operator(eu, ctx, op, first, T, "update_values(sparse tensor) %s %s" % (fmt, pattern))
    # astype of a device-born operator converts on the device
    opc = op.astype(np.complex128)
    assert opc.dtype == np.complex128 and opc.ingest_info["from_device"] and opc.ingest_info["value_bytes_to_host"] == 0
    assert_same_operator(eu, ctx, opc, eu.MIOperator(A.astype(np.complex128), ctx), np.complex128, "astype %s %s" % (fmt, pattern))


# ------------------------------------------------------------------ 6. bad input is an error, not a fault
def test_bad_device_arrays_are_refused_before_anything_indexes_by_them(eu):
    ctx = eu.Context()
    n = 5000
    A = c2_operator(n)
    A.sort_indices()
    b = np.random.default_rng(9).standard_normal(n)
    good = eu.MIOperator(A, ctx)
    w0 = np.array(eu.expv(0.5, good, b, m=20, ishermitian=False, opnorm=1.0))
    lib = eu._lib.load()
    keep = []

    def attempt(fmt, ptr, ind, base, nnz=None, idx_bytes=4, loc=1, idx=np.int32):
        val = np.ones(len(ind))
        arrs = [eu.DeviceArray.from_host(np.asarray(x, dtype=t), ctx) for x, t in ((ptr, idx), (ind, idx), (val, np.float64))]
        keep.extend(arrs)
        h = C.c_void_p()
        fn = lib.expv_mi_op_create_csr_loc if fmt == "csr" else lib.expv_mi_op_create_csc_loc
        rc = fn(ctx._h, 0, n, len(ind) if nnz is None else nnz, arrs[0].ptr, arrs[1].ptr, arrs[2].ptr, idx_bytes, base, loc, C.byref(h))
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.api._check(rc, ctx._h)
        assert ei.value.code == ARGUMENT_ERROR and h.value is None, (ei.value, h.value)
        return str(ei.value)

    ip, ix = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    for fmt, pname, iname in (("csr", "rowptr", "op_create_csr: column index out of range"), ("csc", "colptr", "sparse operator: row index out of range")):
        who = "op_create_" + fmt
        for idx in (np.int32, np.int64):
            bad = ix.copy(); bad[1234] = n
            assert iname in attempt(fmt, ip, bad, 0, idx=idx, idx_bytes=np.dtype(idx).itemsize)
            bad = ix.copy(); bad[len(ix) - 2] = -1
            msg = attempt(fmt, ip, bad, 0, idx=idx, idx_bytes=np.dtype(idx).itemsize)
            assert iname in msg and str(len(ix) - 2) in msg
        bad = ix + 1; bad[77] = 0                                              # base 1: index 0
        assert iname in attempt(fmt, ip + 1, bad, 1)
        bad = ip.copy(); bad[100] = bad[99] - 1                                # decreasing
        assert who + ": " + pname + " must be non-decreasing" in attempt(fmt, bad, ix, 0)
        assert who + ": " + pname + "[0] must equal the index base" in attempt(fmt, ip + 1, ix, 0)
        assert who + ": " + pname + "[0] must equal the index base" in attempt(fmt, ip, ix + 1, 1)
        assert who + ": nnz must equal " + pname + "[n] - index base" in attempt(fmt, ip, ix[:-3], 0)         # stated nnz (the buffer) shorter
        bad = ip.copy(); bad[-1] -= 3
        assert who + ": nnz must equal " + pname + "[n] - index base" in attempt(fmt, bad, ix, 0)          # ptr[n] short of the buffer
        assert who + ": idx_bytes must be 4 or 8" in attempt(fmt, ip, ix, 0, idx_bytes=2)
        assert who + ": bad location" in attempt(fmt, ip, ix, 0, loc=7)
    ctx.sync()
    w1 = np.array(eu.expv(0.5, good, b, m=20, ishermitian=False, opnorm=1.0))
    assert np.array_equal(w0, w1)
    ok = raw_create(eu, ctx, "csr", A, np.int32, 0, 1)                         # and the context still creates operators
    assert np.array_equal(np.array(eu.expv(0.5, ok, b, m=20, ishermitian=False, opnorm=1.0)), w0)


# ------------------------------------------------------------------ 7. unsorted rows: the one case that may download values
def test_unsorted_rows_take_the_host_hermitian_test_and_still_match(eu, torch):
    n = 4000
    A = sprand_gputests(n, seed=5)
    lens = np.diff(A.indptr)
    r = int(np.argmax(lens >= 2))
    k = A.indptr[r]
    ip, ix, va = A.indptr.copy(), A.indices.copy(), A.data.copy()
    ix[[k, k + 1]] = ix[[k + 1, k]]
    va[[k, k + 1]] = va[[k + 1, k]]
    At = torch.sparse_csr_tensor(torch.as_tensor(ip), torch.as_tensor(ix), torch.as_tensor(va), size=A.shape).cuda()
    ctx = eu.Context()
    opd, oph = eu.MIOperator(At, ctx), eu.MIOperator(A, ctx)
    info = opd.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (n + 1 + A.nnz)
    assert info["value_bytes_to_host"] in (0, 16 * A.nnz), info
    assert opd.ishermitian == oph.ishermitian and opd.nnz == oph.nnz
    b = np.random.default_rng(2).standard_normal(n) + 0j
    # (one row is summed in another order: not the same bits; the parity bar of the suite)
    close(eu.expv(0.3, opd, b, m=25), eu.expv(0.3, oph, b, m=25), TOL, "expv, one row unsorted, device-born vs host-born")
    Hs = (A + A.conj().T).tocsr()
    Hs.sort_indices()
    k = Hs.indptr[int(np.argmax(np.diff(Hs.indptr) >= 2))]
    ix, va = Hs.indices.copy(), Hs.data.copy()
    ix[[k, k + 1]] = ix[[k + 1, k]]
    va[[k, k + 1]] = va[[k + 1, k]]
    Ht = torch.sparse_csr_tensor(torch.as_tensor(Hs.indptr), torch.as_tensor(ix), torch.as_tensor(va), size=Hs.shape).cuda()
    assert eu.MIOperator(Ht, ctx).ishermitian and eu.MIOperator(Hs, ctx).ishermitian


# ------------------------------------------------------------------ 8. plan cache
def test_second_device_creation_of_a_pattern_takes_the_plan_from_the_cache(eu, torch):
    A = _shuffle(c2_operator(30_000), 21)
    A.sort_indices()
    At = to_torch_sparse(torch, A)
    ctx = eu.Context()
    eu.plan_cache(clear=True)
    op1 = eu.MIOperator(At, ctx)
    h1 = eu.plan_cache()["hits"]
    A2 = A.copy()
    A2.data = A.data * 1.5
    op2 = eu.MIOperator(to_torch_sparse(torch, A2), ctx)
    assert eu.plan_cache()["hits"] == h1 + 1
    assert op1.reorder_info["reordered"] and op2.reorder_info["reordered"]
    assert not op1.ingest_info["plan_cached"] and op2.ingest_info["plan_cached"]
    assert_same_operator(eu, ctx, op2, eu.MIOperator(A2, ctx), np.float64, "plan from the cache")


# ------------------------------------------------------------------ 9. gputests.jl:41-58, device-resident end to end
def test_reference_gpu_test_device_resident_end_to_end(eu, torch):
    n = 1000
    A = sprand_gputests(n)
    rng = np.random.default_rng(0x0452)
    b = rng.random(n) + 1j * rng.random(n)
    At, bt = to_torch_sparse(torch, A, np.int64), torch.as_tensor(b).cuda()
    w = eu.expv(0.1, At, bt)
    assert torch.is_tensor(w) and w.is_cuda and w.dtype == torch.complex128
    close(w.cpu().numpy(), ko.expv(0.1, A, b), TOL, "gputests.jl:41-58 expv, A and b device-resident, vs oracle")
    ts = np.linspace(0, 1, 300)
    E = eu.expv_timestep(ts.copy(), At, bt)
    assert torch.is_tensor(E) and E.is_cuda
    close(E.cpu().numpy(), ko.expv_timestep(ts.copy(), A, b), TOL, "gputests.jl:41-58 expv_timestep 300 snapshots, device-resident, vs oracle")
    # the other front ends take the tensor too
    Ks = eu.arnoldi(At, bt, m=20)
    close(Ks.getH(), ko.arnoldi(A, b, m=20).getH(), TOL, "arnoldi(device CSR tensor)", mat=True)
    close(eu.phiv(0.2, At, bt, 2, m=20).cpu().numpy(), ko.phiv(0.2, A, b, 2, m=20), 1e-11, "phiv(device CSR tensor)")
    Ar = c2_operator(4000)
    br = rng.standard_normal(4000)
    wk, sk = eu.kiops(1.0, to_torch_sparse(torch, Ar), br, ishermitian=False)
    wko, sko = ko.kiops(1.0, Ar, br, ishermitian=False)
    assert tuple(sk) == tuple(sko), (sk, sko)
    close(wk, wko, 1e-10, "kiops(device CSR tensor)")
    B = np.asfortranarray(rng.standard_normal((4000, 2)))
    U = eu.phiv_timestep(np.array([0.5, 1.0]), to_torch_sparse(torch, Ar), B, tol=1e-8)
    close(U, ko.phiv_timestep(np.array([0.5, 1.0]), Ar, B, tol=1e-8), 1e-10, "phiv_timestep(device CSR tensor)")
    with pytest.raises(TypeError, match="sparse_csr"):
        eu.MIOperator(At.to_sparse_coo())
