"""Sparse operators created from block-compressed arrays (expv_mi_op_create_bsr_loc; MIOperator.from_bsr of a torch.sparse_bsr /
sparse_bsc tensor, a scipy bsr_matrix or three arrays).

Two yardsticks, both compared for bit equality: the operator created on the device from the scalar CSR / CSC arrays the position
contract defines (tests/bsr_cases.py: expand -- held against scipy in tests/test_bsr_operator_cpu.py), and, where the block rows
are sorted, the operator created on the host from the same matrix.  From the checked scalar arrays on a block-born operator IS
the CSR / CSC-born one."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import bsr_cases as bc
from tests._util import stencil2d
from tests.limits import parse_constants
from tests.test_gpu_device_operator import ARGUMENT_ERROR, DTYPES, RawOp, assert_same_operator, sprand_gputests, to_torch_sparse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSR_TILE = parse_constants(open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_bsr.hip")).read())["BSR_TILE"]
CODE = {"float64": 0, "complex128": 1, "float32": 2, "complex64": 3}
ROW_MAJOR, COL_MAJOR, COMPRESSED_COLS = 0, 1, 2


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bsr_op(eu, torch, ctx, ptr, idx, vals, it=np.int64, order="row", compressed="rows", base=0, how="arrays"):
    """a device-born operator of the block arrays (vals row-major, zero-based): through a torch.sparse_bsr / sparse_bsc tensor or
    through from_bsr(ptr, idx, vals) on device tensors in the given block order and index base"""
    n = (len(ptr) - 1) * vals.shape[1]
    if how == "tensor":
        assert order == "row" and base == 0
        mk = torch.sparse_bsr_tensor if compressed == "rows" else torch.sparse_bsc_tensor
        return eu.MIOperator.from_bsr(mk(dev(torch, ptr.astype(it)), dev(torch, idx.astype(it)), dev(torch, vals), size=(n, n)), ctx=ctx)
    return eu.MIOperator.from_bsr(dev(torch, (ptr + base).astype(it)), dev(torch, (idx + base).astype(it)), dev(torch, bc.as_block_order(vals, order)),
                                  index_base=base, compressed=compressed, block_order=order, ctx=ctx)


def twin(eu, ctx, ptr, idx, vals, compressed="rows"):
    """the operator expv_mi_op_create_csr_loc / _csc_loc makes of the restatement's scalar arrays, on the device, entry order kept"""
    bd = vals.shape[1]
    sptr, sidx, sval = bc.expand(ptr, idx, vals, bd, "row", compressed)
    lib = eu._lib.load()
    arrs = [eu.DeviceArray.from_host(sptr.astype(np.int32), ctx)]
    if len(sidx):
        arrs += [eu.DeviceArray.from_host(sidx.astype(np.int32), ctx), eu.DeviceArray.from_host(np.ascontiguousarray(sval), ctx)]
    p = [a.ptr for a in arrs] + [None, None]
    h = C.c_void_p()
    fn = lib.expv_mi_op_create_csr_loc if compressed == "rows" else lib.expv_mi_op_create_csc_loc
    eu.api._check(fn(ctx._h, CODE[vals.dtype.name], len(sptr) - 1, len(sidx), p[0], p[1], p[2], 4, 0, 1, C.byref(h)), ctx._h)
    return RawOp(eu, ctx, h)


def same_everything(eu, ctx, op, ref, T, what, m=25, opnorm=True):
    """n, nnz, ishermitian, path flags, arnoldi / expv / phiv bits (assert_same_operator) + opnorm_inf and matvec bits
    (opnorm=False for a host-born yardstick, whose norm is summed on the host in another order)"""
    n = ref.shape[0]
    if n > 30:
        assert_same_operator(eu, ctx, op, ref, T, what, m=m)
    else:
        assert (op.nnz, op.shape, op.dtype, op.ishermitian) == (ref.nnz, ref.shape, ref.dtype, ref.ishermitian), what
    assert not opnorm or op.opnorm_inf == ref.opnorm_inf, (what, op.opnorm_inf, ref.opnorm_inf)
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(T).kind == "c" else 0)).astype(T)
    assert np.array_equal(np.array(op.matvec(x)), np.array(ref.matvec(x))), what


def ingest(op):
    d = dict(op.ingest_info)
    d.pop("create_s"), d.pop("ingest_s"), d.pop("plan_cached")
    return d


# ------------------------------------------------------------------ 1. same operator, same bits
# every block_dim, element type, index type and way in at least once; every pair of {block order x compression}
COMBOS = [(1, np.float64, np.int32, "row", "rows", "tensor"), (2, np.complex128, np.int64, "col", "rows", "arrays"),
          (3, np.float32, np.int32, "row", "cols", "tensor"), (4, np.complex64, np.int64, "col", "cols", "arrays"),
          (5, np.float64, np.int64, "col", "rows", "arrays"), (8, np.complex128, np.int32, "row", "cols", "arrays"),
          (3, np.float64, np.int64, "row", "rows", "arrays")]
assert {c[1] for c in COMBOS} == set(DTYPES)


@pytest.mark.parametrize("bd,T,it,order,compressed,how", COMBOS)
def test_block_tridiagonal_gives_the_csr_born_and_the_host_born_operator_bit_for_bit(eu, torch, bd, T, it, order, compressed, how):
    nb = 37
    ptr, idx, vals = bc.block_tridiagonal(nb, bd, T)
    A = sp.bsr_matrix((vals, idx, ptr), shape=(nb * bd, nb * bd))
    if compressed == "cols":
        ptr, idx, vals = bc.bsc_of(ptr, idx, vals, bd)
    what = "bd %d %s %s %s %s %s" % (bd, np.dtype(T).name, np.dtype(it).name, order, compressed, how)
    ctx = eu.Context()
    ref = twin(eu, ctx, ptr, idx, vals, compressed)
    op = bsr_op(eu, torch, ctx, ptr, idx, vals, it, order, compressed, how=how)
    n, nnz = nb * bd, len(idx) * bd * bd
    assert op.shape == (n, n) and op.nnz == nnz
    same_everything(eu, ctx, op, ref, T, what)
    info = op.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (n + 1 + nnz) and info["value_bytes_to_host"] == 0, info
    assert info["coo_entries"] == 0 and info["sort_passes"] == 0
    assert ingest(op) == ingest(ref)                       # bd = 1: expv_mi_op_create_csr_loc on the same arrays, in everything
    # the host-born operator of the same matrix
    M = bc.scalar_matrix(ptr, idx, vals, bd, "row", compressed)
    assert np.array_equal(M.toarray(), A.toarray())
    same_everything(eu, ctx, op, eu.MIOperator(M, ctx), T, what + " vs host-born", opnorm=False)


# ------------------------------------------------------------------ 2. it reaches the structured paths
@pytest.mark.parametrize("case", ["two_species_grid", "permuted_block_tridiagonal"])
def test_structured_patterns_take_the_twins_path_and_its_plan(eu, torch, case):
    T = np.float64
    if case == "two_species_grid":
        bd = 2
        ptr, idx, vals = bc.from_block_pattern(stencil2d(64), bd, T, 21)       # kron(grid, ones(2, 2))-shaped, n = 8192
    else:
        bd, nb = 3, 7000
        P = sp.csr_matrix(sp.diags([np.ones(nb - 1), np.ones(nb), np.ones(nb - 1)], [-1, 0, 1]))
        perm = np.random.default_rng(22).permutation(nb)
        ptr, idx, vals = bc.from_block_pattern(P[perm][:, perm], bd, T, 22)
    ctx = eu.Context()
    eu.plan_cache(clear=True)
    ref = twin(eu, ctx, ptr, idx, vals)
    before = eu.plan_cache()
    op = bsr_op(eu, torch, ctx, ptr, idx, vals, how="tensor")
    after = eu.plan_cache()
    print("[bsr] %s: reorder %s patch %s cache %s -> %s" % (case, ref.reorder_info, ref.patch_info, before, after))
    assert_same_operator(eu, ctx, op, ref, T, case)        # reorder_info, patch_info, step form, bits
    # the twin's plan, if it made one, is the one the block-born operator takes
    assert after["hits"] == before["hits"] + (1 if before["plans"] else 0)
    assert op.ingest_info["plan_cached"] == bool(before["plans"]) and not ref.ingest_info["plan_cached"]
    if case == "permuted_block_tridiagonal":
        assert ref.reorder_info["reordered"] and op.reorder_info["reordered"] and op.ingest_info["plan_cached"]


# ------------------------------------------------------------------ 3. shapes that break an expansion kernel
SMALL = [np.float64, np.complex64]


@pytest.mark.parametrize("T", SMALL + [np.float32, np.complex128])
def test_one_block_larger_than_a_workgroup(eu, torch, T):
    bd = 70                                                # 4900 elements in one block, one block row
    ptr, idx = np.array([0, 1]), np.array([0])
    vals = bc.random_values((1, bd, bd), T, np.random.default_rng(30))
    ctx = eu.Context()
    for order in ("row", "col"):
        for compressed in ("rows", "cols"):
            op = bsr_op(eu, torch, ctx, ptr, idx, vals, np.int32, order, compressed)
            assert op.nnz == bd * bd
            same_everything(eu, ctx, op, twin(eu, ctx, ptr, idx, vals, compressed), T, "one 70 x 70 block %s %s" % (order, compressed))
            x = np.ones(bd, dtype=T)
            assert np.allclose(np.array(op.matvec(x)), vals[0] @ x, rtol=1e-4)


@pytest.mark.parametrize("T", SMALL)
def test_one_by_one_and_the_zero_operator(eu, torch, T):
    ctx = eu.Context()
    op = bsr_op(eu, torch, ctx, np.array([0, 1]), np.array([0]), np.array([[[2.5]]], dtype=T))
    assert op.shape == (1, 1) and op.nnz == 1 and np.array_equal(np.array(op.matvec(np.ones(1, dtype=T))), np.array([2.5], dtype=T))
    for bd in (1, 3):
        nb = 5
        z = bsr_op(eu, torch, ctx, np.zeros(nb + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, bd, bd), dtype=T))
        assert z.shape == (nb * bd, nb * bd) and z.nnz == 0 and z.opnorm_inf == 0.0
        x = np.arange(1, nb * bd + 1).astype(T)
        assert np.array_equal(np.array(z.matvec(x)), np.zeros(nb * bd, dtype=T))


@pytest.mark.parametrize("compressed", ["rows", "cols"])
@pytest.mark.parametrize("T", SMALL)
def test_empty_block_rows_and_one_block_row_that_holds_everything(eu, torch, T, compressed):
    ctx = eu.Context()
    bd, nb = 3, 40
    ptr, idx, vals = bc.with_empty_block_rows(nb, bd, T, seed=31)
    cnt = np.diff(ptr)
    assert cnt[0] == 0 and cnt[1] == 0 and np.all(cnt[5:8] == 0) and cnt[10] == 0 and cnt[-1] == 0 and cnt[-2] == 0
    if compressed == "cols":
        ptr, idx, vals = bc.bsc_of(ptr, idx, vals, bd)
    op = bsr_op(eu, torch, ctx, ptr, idx, vals, np.int32, "col", compressed)
    same_everything(eu, ctx, op, twin(eu, ctx, ptr, idx, vals, compressed), T, "empty block rows " + compressed)
    # every block of the matrix in block row 17
    ptr1 = np.zeros(nb + 1, dtype=np.int64)
    ptr1[18:] = nb
    idx1 = np.arange(nb, dtype=np.int64)
    vals1 = bc.random_values((nb, bd, bd), T, np.random.default_rng(32))
    op = bsr_op(eu, torch, ctx, ptr1, idx1, vals1, np.int64, "row", compressed, how="tensor")
    same_everything(eu, ctx, op, twin(eu, ctx, ptr1, idx1, vals1, compressed), T, "one full block row " + compressed)


# entry counts one below, at and one above the tile of k_bsr_idx / k_bsr_vals, and past two tiles; block_dim 3 moves in whole
# blocks of 9 entries (BSR_TILE is a multiple of 9), so its neighbours of the tile are one BLOCK below and above
@pytest.mark.parametrize("bd,nnzb", [(1, BSR_TILE - 1), (1, BSR_TILE), (1, BSR_TILE + 1), (1, 2 * BSR_TILE + 1),
                                     (3, BSR_TILE // 9 - 1), (3, BSR_TILE // 9), (3, BSR_TILE // 9 + 1), (3, 2 * BSR_TILE // 9 + 1)])
@pytest.mark.parametrize("T", SMALL)
def test_entry_counts_around_the_tile(eu, torch, T, bd, nnzb):
    assert BSR_TILE % 9 == 0
    nb = 300
    rng = np.random.default_rng(33)
    cnt = rng.multinomial(nnzb, np.ones(nb) / nb)
    cnt = np.minimum(cnt, nb)
    cnt[0] += nnzb - cnt.sum()                              # (a few blocks may have been cut off above)
    assert cnt.max() <= nb
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(nb, c, replace=False)) for c in cnt]).astype(np.int64)
    vals = bc.random_values((nnzb, bd, bd), T, rng)
    ctx = eu.Context()
    for order in ("row", "col"):
        op = bsr_op(eu, torch, ctx, ptr, idx, vals, np.int32, order)
        assert op.nnz == nnzb * bd * bd
        same_everything(eu, ctx, op, twin(eu, ctx, ptr, idx, vals), T, "bd %d, %d blocks, %s" % (bd, nnzb, order))


@pytest.mark.parametrize("T,it", [(np.float64, np.int64), (np.float32, np.int32), (np.complex64, np.int32)])
def test_arrays_that_start_one_element_into_their_storage_and_index_base_one(eu, torch, T, it):
    """fp64 / int64 / complex64 slices are 8-byte aligned, fp32 / int32 slices 4-byte aligned: never on 16 bytes"""
    ctx = eu.Context()
    for bd in (2, 4):                                       # 4: the wide loads would apply, were the address aligned
        ptr, idx, vals = bc.block_tridiagonal(50, bd, T, seed=34)
        ref = twin(eu, ctx, ptr, idx, vals)
        P = dev(torch, np.concatenate([[7], ptr + 1]).astype(it))[1:]
        I = dev(torch, np.concatenate([[7], idx + 1]).astype(it))[1:]
        V = dev(torch, np.concatenate([np.full(1, 7, dtype=T), vals.ravel()]))[1:].reshape(len(idx), bd, bd)
        for t in (P, I, V):
            assert t.data_ptr() % 16 != 0 and t.data_ptr() % t.element_size() == 0
        op = eu.MIOperator.from_bsr(P, I, V, index_base=1, ctx=ctx)
        same_everything(eu, ctx, op, ref, T, "offset slices, base 1, bd %d" % bd)
        # ... and the aligned arrays (the wide loads of bd = 4) give the same operator
        same_everything(eu, ctx, bsr_op(eu, torch, ctx, ptr, idx, vals, it), ref, T, "aligned, bd %d" % bd)
        V2 = dev(torch, np.concatenate([np.full(1, 7, dtype=T), 2 * vals.ravel()]))[1:]
        op.update_values(V2)                                # a refresh from an offset slice
        same_everything(eu, ctx, op, twin(eu, ctx, ptr, idx, 2 * vals), T, "offset refresh, bd %d" % bd)


# ------------------------------------------------------------------ 4. unsorted and repeated blocks
@pytest.mark.parametrize("compressed", ["rows", "cols"])
@pytest.mark.parametrize("T", SMALL)
def test_block_rows_in_reverse_order_with_a_repeated_block(eu, torch, T, compressed):
    bd, nb = 3, 37
    ptr, idx, vals = bc.reverse_block_rows(*bc.block_tridiagonal(nb, bd, T, seed=40))
    idx = idx.copy()
    idx[ptr[20]] = idx[ptr[20] + 1]                         # block row 20 names one block column twice
    ctx = eu.Context()
    ref = twin(eu, ctx, ptr, idx, vals, compressed)
    op = bsr_op(eu, torch, ctx, ptr, idx, vals, np.int64, "row", compressed, how="tensor")
    assert op.nnz == len(idx) * bd * bd
    same_everything(eu, ctx, op, ref, T, "reversed + repeated " + compressed)
    assert ingest(op) == ingest(ref)
    if compressed == "rows":                                # rows out of order: the Hermitian test ran on a downloaded copy
        assert op.ingest_info["value_bytes_to_host"] > 0, op.ingest_info


# ------------------------------------------------------------------ 5. Hermitian
@pytest.mark.parametrize("T", [np.complex128, np.float64, np.complex64])
def test_hermitian_matrix_as_column_major_bsc(eu, torch, T):
    bd, nb = 3, 60
    ptr, idx, vals = bc.block_tridiagonal(nb, bd, T, seed=50)
    n = nb * bd
    A = sp.bsr_matrix((vals, idx, ptr), shape=(n, n))
    Hm = (A + A.conj().T).tobsr(blocksize=(bd, bd))
    Hm.sort_indices()
    hp, hi, hv = Hm.indptr.astype(np.int64), Hm.indices.astype(np.int64), Hm.data
    cp, ci, cv = bc.bsc_of(hp, hi, hv, bd)
    ctx = eu.Context()
    op = bsr_op(eu, torch, ctx, cp, ci, cv, np.int32, "col", "cols")
    ref = twin(eu, ctx, hp, hi, hv)                        # the CSR-born operator of the same matrix
    assert op.ishermitian and ref.ishermitian
    rng = np.random.default_rng(51)
    b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if np.dtype(T).kind == "c" else 0)).astype(T)
    w1 = np.array(eu.expv(0.3, op, b, m=20))
    p1 = tuple(eu.expv.last_stats["path"])
    w2 = np.array(eu.expv(0.3, ref, b, m=20))
    assert p1 == tuple(eu.expv.last_stats["path"]) and np.array_equal(w1, w2)
    op.update_values(np.triu(np.ones((bd, bd)))[None] * bc.as_block_order(cv, "col"))      # no longer Hermitian
    assert not op.ishermitian


# ------------------------------------------------------------------ 6. update_values
@pytest.mark.parametrize("order,compressed", [("row", "rows"), ("col", "rows"), ("row", "cols"), ("col", "cols")])
@pytest.mark.parametrize("T", SMALL)
def test_update_values_in_block_order_is_creating_anew(eu, torch, T, order, compressed):
    bd, nb = 3, 37
    ptr, idx, vals = bc.with_empty_block_rows(nb, bd, T, seed=60)
    rng = np.random.default_rng(61)
    v2, v3 = bc.random_values(vals.shape, T, rng), 3 * bc.random_values(vals.shape, T, rng)
    ctx = eu.Context()
    op = bsr_op(eu, torch, ctx, ptr, idx, vals, np.int64, order, compressed)
    n0 = op.opnorm_inf
    op.update_values(dev(torch, bc.as_block_order(v2, order)))                      # a device tensor, (nnzb, bd, bd)
    same_everything(eu, ctx, op, bsr_op(eu, torch, ctx, ptr, idx, v2, np.int64, order, compressed), T, "refresh from the device")
    assert op.opnorm_inf != n0
    op.update_values(bc.as_block_order(v3, order).ravel())                          # a host array, flat
    same_everything(eu, ctx, op, twin(eu, ctx, ptr, idx, v3, compressed), T, "refresh from the host")
    with pytest.raises(eu.DimensionMismatch):
        op.update_values(v2.ravel()[:-1])
    with pytest.raises(eu.DimensionMismatch):
        op.update_values(dev(torch, v2.ravel()[: len(idx) * bd]))
    opc = op.astype(np.complex128)                                                  # rebuilt from the kept parts, on the device
    assert opc.dtype == np.complex128 and opc.ingest_info["from_device"] and opc.nnz == op.nnz
    same_everything(eu, ctx, opc, twin(eu, ctx, ptr, idx, v3.astype(np.complex128), compressed), np.complex128, "astype")


def test_update_values_from_a_tensor_wants_the_indices_of_the_creation(eu, torch):
    T, bd, nb = np.float64, 2, 37
    ptr, idx, vals = bc.block_tridiagonal(nb, bd, T, seed=62)
    n = nb * bd

    def tensor(i, v):
        return torch.sparse_bsr_tensor(dev(torch, ptr), dev(torch, i), dev(torch, v), size=(n, n))

    ctx = eu.Context()
    op = eu.MIOperator.from_bsr(tensor(idx, vals), ctx=ctx)
    Hs = sp.bsr_matrix((vals + vals.transpose(0, 2, 1), idx, ptr), shape=(n, n))
    Hs = (Hs + Hs.T).tobsr(blocksize=(bd, bd))
    Hs.sort_indices()
    assert np.array_equal(Hs.indices, idx) and not op.ishermitian
    op.update_values(tensor(idx, Hs.data))                                          # same indices: symmetric values now
    assert op.ishermitian
    same_everything(eu, ctx, op, twin(eu, ctx, ptr, idx, Hs.data), T, "refresh from a BSR tensor")
    other = idx.copy()
    other[[0, 1]] = other[[1, 0]]
    with pytest.raises(ValueError):
        op.update_values(tensor(other, vals))
    with pytest.raises(ValueError):
        op.update_values(torch.sparse_bsc_tensor(dev(torch, ptr), dev(torch, idx), dev(torch, vals), size=(n, n)))
    with pytest.raises(TypeError, match="from_bsr"):
        eu.MIOperator(tensor(idx, vals), ctx)                                       # the plain constructor keeps to CSR / CSC


# ------------------------------------------------------------------ 7. refusals
def test_bad_block_arrays_are_refused_in_the_host_creators_words(eu, torch):
    lib = eu._lib.load()
    ctx = eu.Context()
    bd, nb = 2, 12
    ptr0, idx0, vals0 = bc.block_tridiagonal(nb, bd, np.float64, seed=70)
    n, nnzb = nb * bd, len(idx0)
    good = bsr_op(eu, torch, ctx, ptr0, idx0, vals0)
    b = np.random.default_rng(71).standard_normal(n)
    w0 = np.array(eu.expv(0.5, good, b, m=10, ishermitian=False, opnorm=1.0))
    keep = []

    def attempt(ptr=ptr0, idx=idx0, n=n, nnzb=nnzb, bd=bd, layout=ROW_MAJOR, idx_bytes=8, base=0, loc=1, null_vals=False, it=np.int64):
        arrs = [eu.DeviceArray.from_host(np.ascontiguousarray(x), ctx) for x in (ptr.astype(it), idx.astype(it), vals0)]
        keep.extend(arrs)
        h = C.c_void_p()
        rc = lib.expv_mi_op_create_bsr_loc(ctx._h, 0, n, nnzb, bd, arrs[0].ptr, arrs[1].ptr, None if null_vals else arrs[2].ptr, idx_bytes, base,
                                           layout, loc, C.byref(h))
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.api._check(rc, ctx._h)
        assert ei.value.code == ARGUMENT_ERROR and h.value is None, (ei.value, h.value)
        return str(ei.value)

    p = ptr0.copy()
    p[0] = 1
    assert "op_create_bsr: rowptr[0] must equal the index base" in attempt(ptr=p)
    assert "op_create_bsr: colptr[0] must equal the index base" in attempt(ptr=p, layout=COMPRESSED_COLS)
    p = ptr0.copy()
    p[5] = p[4] - 1
    said = attempt(ptr=p)
    assert "op_create_bsr: rowptr must be non-decreasing" in said and "(first at position 5)" in said, said
    assert "op_create_bsr: nnzb must equal rowptr[n / block_dim] - index base" in attempt(nnzb=nnzb - 1)
    for bad in (nb, -1):                    # nb * bd + c would be a legal scalar column for c < ... : the range is nb, not n
        i = idx0.copy()
        i[[9, 20]] = bad
        for it, ib in ((np.int64, 8), (np.int32, 4)):
            said = attempt(idx=i, it=it, idx_bytes=ib)
            assert "op_create_bsr: column index out of range" in said and "(first at position 9)" in said, said
        said = attempt(idx=i, layout=COMPRESSED_COLS | COL_MAJOR)
        assert "row index out of range" in said and "(first at position 9)" in said, said
    assert "op_create_bsr: n must be a multiple of block_dim" in attempt(n=n + 1)
    assert "op_create_bsr: block_dim must be at least 1" in attempt(bd=0)
    assert "op_create_bsr: unknown layout bits" in attempt(layout=4)
    assert "op_create_bsr: idx_bytes must be 4 or 8" in attempt(idx_bytes=2)
    assert "op_create_bsr: negative nnzb" in attempt(nnzb=-1)
    assert "op_create_bsr: bad location" in attempt(loc=7)
    assert "op_create_bsr: null colind / vals" in attempt(null_vals=True)
    # nnzb * block_dim^2 = 2^32 past CSR32: found before the null values are (and before anything could be read)
    said = attempt(ptr=np.array([0, 1]), idx=np.array([0]), n=65536, nnzb=1, bd=65536, null_vals=True)
    assert "CSR32" in said and "op_create_bsr" in said, said
    assert lib.expv_mi_op_create_bsr_loc(ctx._h, 0, n, 0, bd, None, None, None, 8, 0, 0, 1, None) == ARGUMENT_ERROR      # null output
    ctx.sync()
    w1 = np.array(eu.expv(0.5, good, b, m=10, ishermitian=False, opnorm=1.0))
    assert np.array_equal(w0, w1)           # and the context is as good as before


# ------------------------------------------------------------------ 8. gputests.jl:41-58 with a block-sparse tensor
def test_reference_gpu_test_shape_as_a_bsr_tensor(eu, torch):
    n = 1000
    A = sprand_gputests(n)
    rng = np.random.default_rng(0x0452)
    bt = torch.as_tensor(rng.random(n) + 1j * rng.random(n)).cuda()
    Ab = to_torch_sparse(torch, A, np.int64, device="cpu").to_sparse_bsr((2, 2))
    ptr, idx, vals = Ab.crow_indices().numpy(), Ab.col_indices().numpy(), Ab.values().numpy()
    Ab = torch.sparse_bsr_tensor(dev(torch, ptr), dev(torch, idx), dev(torch, vals), size=(n, n))
    E = bc.scalar_matrix(ptr, idx, vals, 2)                 # the expanded matrix: zeros inside the blocks stored
    assert E.nnz == 4 * len(idx) > A.nnz and np.array_equal(E.toarray(), A.toarray())
    Ec = to_torch_sparse(torch, E, np.int64)
    w = eu.expv(0.1, Ab, bt)
    assert torch.is_tensor(w) and w.is_cuda and w.dtype == torch.complex128
    assert torch.equal(w, eu.expv(0.1, Ec, bt))
    ts = np.linspace(0, 1, 300)
    assert torch.equal(eu.expv_timestep(ts.copy(), Ab, bt), eu.expv_timestep(ts.copy(), Ec, bt))
    assert torch.equal(eu.phiv(0.2, Ab, bt, 2, m=20), eu.phiv(0.2, Ec, bt, 2, m=20))


# ------------------------------------------------------------------ 9. loc = HOST gives the bits of loc = DEVICE
@pytest.mark.parametrize("T", SMALL)
def test_host_data_is_staged_and_takes_the_same_path(eu, torch, T):
    bd, nb = 3, 37
    ptr, idx, vals = bc.reverse_block_rows(*bc.with_empty_block_rows(nb, bd, T, seed=90))
    S = sp.bsr_matrix((vals, idx.astype(np.int32), ptr.astype(np.int32)), shape=(nb * bd, nb * bd))
    ctx = eu.Context()
    oph = eu.MIOperator.from_bsr(S, ctx=ctx)
    opd = bsr_op(eu, torch, ctx, ptr, idx, vals, np.int32)
    assert oph.ingest_info["from_device"] and ingest(oph) == ingest(opd)
    same_everything(eu, ctx, oph, opd, T, "scipy bsr_matrix vs device tensors")
    # a CPU torch tensor and numpy arrays in column-major BSC go the same way
    cp, ci, cv = bc.bsc_of(*bc.with_empty_block_rows(nb, bd, T, seed=90), bd)
    opn = eu.MIOperator.from_bsr(cp, ci, bc.as_block_order(cv, "col"), compressed="cols", block_order="col", ctx=ctx)
    same_everything(eu, ctx, opn, bsr_op(eu, torch, ctx, cp, ci, cv, np.int64, "col", "cols"), T, "numpy BSC vs device tensors")
    tc = torch.sparse_bsc_tensor(torch.as_tensor(cp), torch.as_tensor(ci), torch.as_tensor(cv), size=(nb * bd, nb * bd))
    same_everything(eu, ctx, eu.MIOperator.from_bsr(tc, ctx=ctx), opn, T, "CPU BSC tensor")
    oph.update_values(S.data * 2)
    same_everything(eu, ctx, oph, twin(eu, ctx, ptr, idx, vals * 2), T, "host refresh")
