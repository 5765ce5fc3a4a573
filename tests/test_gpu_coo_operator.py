"""Sparse operators created from coordinate triplets (expv_mi_op_create_coo_loc; MIOperator.from_coo of a torch.sparse_coo tensor
or of three arrays): any order, repeats added in entry order.

The yardsticks are the operator created on the host from the matrix the contract defines (tests/coo_cases.py: expected_csr; for
exact splits that is the original matrix) and, for sorted input, the operator created from the same CSR arrays on the device.
From the checked CSR arrays on a triplet-born operator IS such an operator, so everything is compared for bit equality."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_oracle as ko
from tests import coo_cases as cc
from tests._util import c2_operator, close
from tests.limits import parse_constants
from tests.test_gpu_device_operator import (ARGUMENT_ERROR, DTYPES, PATTERNS, RawOp, assert_same_operator, make_pattern, sprand_gputests,
                                            to_torch_sparse)
from tests.test_gpu_parity import TOL, _shuffle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COO_TILE = parse_constants(open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_coo.hip")).read())["COO_TILE"]


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def coo_tensor(torch, row, col, vals, n, device="cuda"):
    return torch.sparse_coo_tensor(torch.as_tensor(np.vstack([row, col]).astype(np.int64)), torch.as_tensor(vals), size=(n, n)).to(device)


def from_triplets(eu, torch, ctx, row, col, vals, n, idx=np.int64, how="tensor"):
    """a device-born operator of the triplets: through the torch.sparse_coo tensor (int64 indices are torch's) or from_coo"""
    if how == "tensor" and idx == np.int64:
        return eu.MIOperator.from_coo(coo_tensor(torch, row, col, vals, n), ctx=ctx)
    r, c = torch.as_tensor(row.astype(idx)).cuda(), torch.as_tensor(col.astype(idx)).cuda()
    return eu.MIOperator.from_coo(r, c, torch.as_tensor(vals).cuda(), n, ctx=ctx)


def dense_of(op):
    """the stored matrix, column by column (a column of A is A e_j exactly)"""
    n = op.shape[0]
    E = np.eye(n, dtype=op.dtype)
    return np.column_stack([np.array(op.matvec(np.ascontiguousarray(E[:, j]))) for j in range(n)])


def assert_is_expected(eu, ctx, op, E, T, what):
    """the operator against the expected CSR matrix: exactly"""
    n = E.shape[0]
    assert op.nnz == E.nnz and op.shape == E.shape, (what, op.nnz, E.nnz)
    if n <= 64:
        got = dense_of(op)
        assert np.array_equal(got, E.toarray()), (what, float(np.max(np.abs(got - E.toarray()))))
    else:
        assert_same_operator(eu, ctx, op, eu.MIOperator(E, ctx), T, what)


# ------------------------------------------------------------------ 1. same operator, same bits
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_shuffled_triplets_with_exact_repeats_give_the_host_born_operator_bit_for_bit(eu, torch, pattern, T, idx):
    A = make_pattern(pattern, T)
    n = A.shape[0]
    row, col, vals = cc.split_triplets(A, 0.15, "exact", 31)
    assert len(row) > A.nnz
    ctx = eu.Context()
    oph = eu.MIOperator(A, ctx)
    opd = from_triplets(eu, torch, ctx, row, col, vals, n, idx)
    if pattern == "grid":
        assert oph.patch_info["patch_form"] and opd.patch_info["patch_form"]
    if pattern == "c2_permuted":
        assert oph.reorder_info["reordered"] and opd.reorder_info["reordered"]
    assert_same_operator(eu, ctx, opd, oph, T, "coo %s %s %s" % (pattern, np.dtype(T).name, np.dtype(idx).name))
    info = opd.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (n + 1 + A.nnz) and info["value_bytes_to_host"] == 0, info
    assert info["coo_entries"] == len(row) and info["sort_passes"] > 0, info


# ------------------------------------------------------------------ 2. the smallest shapes that can break a stage
SMALL = [np.float64, np.complex64]


@pytest.mark.parametrize("T", SMALL)
def test_one_by_one(eu, torch, T):
    ctx = eu.Context()
    for count in (1, 300):                 # 300: one cell receives everything -- the long-segment form
        row, col, vals = cc.random_triplets(1, count, T, 40 + count)
        E = cc.expected_csr(row, col, vals, 1)
        op = from_triplets(eu, torch, ctx, row, col, vals, 1)
        assert op.nnz == 1 and op.ingest_info["coo_entries"] == count and op.ingest_info["sort_passes"] == 0
        assert_is_expected(eu, ctx, op, E, T, "n = 1, %d entries" % count)


@pytest.mark.parametrize("T", SMALL)
def test_more_entries_than_cells(eu, torch, T):
    ctx = eu.Context()
    row, col, vals = cc.random_triplets(37, 5000, T, 41)
    E = cc.expected_csr(row, col, vals, 37)
    assert E.nnz <= 37 * 37 and np.max(np.bincount(row * 37 + col)) <= 32      # segments straddle tiles; all of them short
    op = from_triplets(eu, torch, ctx, row, col, vals, 37)
    assert_is_expected(eu, ctx, op, E, T, "n = 37, 5000 entries")
    # ... and with one cell that takes a long segment among the short ones
    row[::9], col[::9] = 17, 5
    E = cc.expected_csr(row, col, vals, 37)
    assert_is_expected(eu, ctx, from_triplets(eu, torch, ctx, row, col, vals, 37), E, T, "n = 37, one long segment")


@pytest.mark.parametrize("ends", [True, False])
@pytest.mark.parametrize("n", [257, 65537])
@pytest.mark.parametrize("T", SMALL)
def test_index_fields_one_bit_past_a_digit_and_runs_of_empty_rows(eu, torch, T, n, ends):
    """n = 2^8 + 1 and 2^16 + 1; ends: entries at (0, 0) and (n - 1, n - 1); otherwise the first and the last rows are empty"""
    ctx = eu.Context()
    row, col, vals = cc.random_triplets(n, 40_000, T, 42, repeat_share=0.1, lo=0 if ends else 5, hi=n if ends else n - 7, ends=ends)
    if n == 257:                            # runs of empty rows inside, too
        keep = (row < 100) | (row > 140)
        row, col, vals = row[keep], col[keep], vals[keep]
    E = cc.expected_csr(row, col, vals, n)
    lens = np.diff(E.indptr)
    assert (lens[0] > 0 and lens[-1] > 0) if ends else (lens[0] == 0 and lens[-1] == 0)
    assert np.any(lens[1:-1] == 0) and E.nnz < len(row)
    op = from_triplets(eu, torch, ctx, row, col, vals, n)
    assert op.ingest_info["sort_passes"] == (4 if n == 257 else 6)      # ceil(9 / 8) resp. ceil(17 / 8) digits per field
    assert_is_expected(eu, ctx, op, E, T, "n = %d ends = %s" % (n, ends))


@pytest.mark.parametrize("count", [COO_TILE - 1, COO_TILE, COO_TILE + 1, 2 * COO_TILE + 1])
@pytest.mark.parametrize("T", SMALL)
def test_entry_counts_around_the_sort_tile(eu, torch, T, count):
    ctx = eu.Context()
    row, col, vals = cc.random_triplets(500, count, T, 43 + count)
    E = cc.expected_csr(row, col, vals, 500)
    for idx in (np.int32, np.int64):
        op = from_triplets(eu, torch, ctx, row, col, vals, 500, idx, how="arrays")
        assert op.ingest_info["coo_entries"] == count
        assert_is_expected(eu, ctx, op, E, T, "n = 500, %d entries, %s" % (count, np.dtype(idx).name))


@pytest.mark.parametrize("T", SMALL)
def test_odd_entry_count_reversed_input_and_adjacent_repeats(eu, torch, T):
    ctx = eu.Context()
    n = 300
    row, col, vals = cc.random_triplets(n, 4001, T, 44)
    t = coo_tensor(torch, row, col, vals, n)
    assert t._indices()[1].data_ptr() % 16 == 8                 # the second index row of an odd count: 8-byte aligned only
    E = cc.expected_csr(row, col, vals, n)
    assert_is_expected(eu, ctx, eu.MIOperator.from_coo(t, ctx=ctx), E, T, "odd entry count through the tensor")
    # reverse sorted order
    order = np.lexsort((col, row))[::-1]
    op = from_triplets(eu, torch, ctx, row[order], col[order], vals[order], n)
    assert op.ingest_info["sort_passes"] > 0
    assert_is_expected(eu, ctx, op, cc.expected_csr(row[order], col[order], vals[order], n), T, "reverse sorted")
    # sorted, with adjacent repeats: nothing to sort (the header's promise), the sums still run
    order = np.lexsort((col, row))
    op = from_triplets(eu, torch, ctx, row[order], col[order], vals[order], n)
    info = op.ingest_info
    assert info["sort_passes"] == 0 and info["coo_entries"] == 4001 and op.nnz == E.nnz < 4001
    assert_is_expected(eu, ctx, op, E, T, "sorted with adjacent repeats")
    v2 = (vals * 1.25).astype(T)
    op.update_values(v2[order])                                 # (one value per triplet, in the order the triplets were handed over)
    assert_is_expected(eu, ctx, op, cc.expected_csr(row[order], col[order], v2[order], n), T, "sorted with adjacent repeats, refreshed")


def test_no_entries_is_the_zero_operator(eu, torch):
    ctx = eu.Context()
    e = np.zeros(0, dtype=np.int64)
    for op in (eu.MIOperator.from_coo(e, e, np.zeros(0), 5, ctx=ctx),
               eu.MIOperator.from_coo(torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.float64), size=(5, 5)).cuda(), ctx=ctx)):
        assert op.nnz == 0 and op.shape == (5, 5) and op.opnorm_inf == 0.0
        b = np.arange(1.0, 6.0)
        assert np.array_equal(np.array(op.matvec(b)), np.zeros(5))
        # exp(0) b = b: the Krylov evaluation normalises b and scales it back, two roundings of each component
        w = np.array(eu.expv(0.5, op, b))
        assert np.all(np.abs(w - b) <= 2 * np.finfo(np.float64).eps * np.abs(b)), w - b


# ------------------------------------------------------------------ 3. sorted, unique input skips the sort
@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_sorted_unique_triplets_skip_the_sort_and_equal_the_csr_born_operator(eu, torch, T):
    A = make_pattern("c2_permuted", T)
    n = A.shape[0]
    ctx = eu.Context()
    opc = eu.MIOperator(to_torch_sparse(torch, A, np.int64), ctx)
    Cm = A.tocoo()
    t = coo_tensor(torch, Cm.row, Cm.col, Cm.data, n).coalesce()
    assert t.is_coalesced()
    for what, op in (("coalesced tensor", eu.MIOperator.from_coo(t, ctx=ctx)),
                     ("tocoo() through from_coo, one-based int32", eu.MIOperator.from_coo(
                         torch.as_tensor((Cm.row + 1).astype(np.int32)).cuda(), torch.as_tensor((Cm.col + 1).astype(np.int32)).cuda(),
                         torch.as_tensor(Cm.data).cuda(), n, index_base=1, ctx=ctx))):
        info = op.ingest_info
        assert info["sort_passes"] == 0 and info["coo_entries"] == A.nnz and info["value_bytes_to_host"] == 0, (what, info)
        assert op.opnorm_inf == opc.opnorm_inf
        assert_same_operator(eu, ctx, op, opc, T, what)
    # new values where they lie: update_values is the CSR one
    op.update_values(torch.as_tensor(Cm.data * 2).cuda())
    A2 = A.copy()
    A2.data = A.data * 2
    assert_same_operator(eu, ctx, op, eu.MIOperator(A2, ctx), T, "sorted unique, refreshed")


# ------------------------------------------------------------------ 4. the order of the sum
def test_entries_of_a_cell_are_added_in_entry_order(eu, torch):
    ctx = eu.Context()
    tiny = 2.0 ** -60
    for parts, want in (((1.0, tiny, -1.0), 0.0), ((1.0, -1.0, tiny), tiny)):
        # other cells around it, listed before, between and after the three parts
        row = np.array([2, 1, 0, 1, 3, 1, 2], dtype=np.int64)
        col = np.array([2, 2, 0, 2, 1, 2, 0], dtype=np.int64)
        vals = np.array([5.0, parts[0], 7.0, parts[1], 3.0, parts[2], 9.0])
        for how in ("tensor", "arrays"):
            op = from_triplets(eu, torch, ctx, row, col, vals, 4, how=how)
            D = dense_of(op)
            assert D[1, 2] == want, (parts, D[1, 2])
            assert op.nnz == 5                                   # a cell that sums to zero stays stored
            assert D[2, 2] == 5.0 and D[0, 0] == 7.0 and D[3, 1] == 3.0 and D[2, 0] == 9.0
        # the host location takes the same path
        oph = eu.MIOperator.from_coo(row, col, vals, 4, ctx=ctx)
        assert np.array_equal(dense_of(oph), D) and oph.nnz == 5
    # ... and through the long-segment form: 200 parts whose left-to-right sum is exact and whose reversed sum is not
    k = 200
    vals = np.concatenate([[1.0], np.full(k - 2, tiny), [-1.0]])
    z = np.zeros(k, dtype=np.int64)
    op = from_triplets(eu, torch, ctx, z, z, vals, 2)
    assert dense_of(op)[0, 0] == 0.0 and op.nnz == 1
    late = np.concatenate([np.full(k - 2, tiny), [1.0, -1.0]])               # the small parts first: they add up before the 1 arrives
    want = cc.expected_csr(z, z, late, 2).data[0]
    assert want == 2.0 ** -52
    assert dense_of(from_triplets(eu, torch, ctx, z, z, late, 2))[0, 0] == want


@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_a_hermitian_matrix_delivered_as_shuffled_triplets_is_hermitian(eu, torch, T):
    n = 3000
    rng = np.random.default_rng(17)
    R = sp.random(n, n, density=8 / n, random_state=rng, dtype=np.float64)
    if np.dtype(T).kind == "c":
        R = R + 1j * sp.random(n, n, density=8 / n, random_state=rng, dtype=np.float64)
    Hm = (R + R.conj().T + sp.diags([rng.standard_normal(n)], [0])).tocsr().astype(T)
    Hm.sort_indices()
    G = (Hm + sp.triu(R, 1).astype(T)).tocsr()
    G.sort_indices()
    ctx = eu.Context()
    for M, herm in ((Hm, True), (G, False)):
        row, col, vals = cc.split_triplets(M, 0.2, "exact", 5)
        op = from_triplets(eu, torch, ctx, row, col, vals, n)
        assert op.ishermitian == herm and op.nnz == M.nnz and op.ingest_info["value_bytes_to_host"] == 0


# ------------------------------------------------------------------ 5. values refreshed in triplet order
@pytest.mark.parametrize("pattern", ["c2", "c2_permuted", "powerlaw"])
def test_update_values_in_triplet_order_equals_creating_anew(eu, torch, pattern):
    T = np.float64
    A = make_pattern(pattern, T)
    n = A.shape[0]
    row, col, vals = cc.split_triplets(A, 0.15, "random", 8)
    ctx = eu.Context()
    op = from_triplets(eu, torch, ctx, row, col, vals, n)
    assert op.reorder_info["reordered"] == (pattern == "c2_permuted") and op.nnz == A.nnz
    v2 = vals * (1.0 + 0.3 * np.cos(np.arange(len(vals))))
    fresh = from_triplets(eu, torch, ctx, row, col, v2, n)
    op.update_values(v2)                                                    # a host array
    assert op.opnorm_inf == fresh.opnorm_inf and op.ishermitian == fresh.ishermitian
    assert_same_operator(eu, ctx, op, fresh, T, "update_values(host array) %s" % pattern)
    assert_same_operator(eu, ctx, op, eu.MIOperator(cc.expected_csr(row, col, v2, n), ctx), T, "update_values vs expected %s" % pattern)
    op.update_values(torch.as_tensor(vals).cuda())                          # a device tensor: back to the first values
    first = from_triplets(eu, torch, ctx, row, col, vals, n)
    assert_same_operator(eu, ctx, op, first, T, "update_values(device tensor) %s" % pattern)
    op.update_values(coo_tensor(torch, row, col, v2, n))                    # a COO tensor with the same indices
    assert_same_operator(eu, ctx, op, fresh, T, "update_values(coo tensor) %s" % pattern)
    with pytest.raises(eu.DimensionMismatch):
        op.update_values(v2[:-1])
    with pytest.raises(eu.DimensionMismatch):
        op.update_values(np.ones(op.nnz))                                   # one per stored entry is not one per triplet
    with pytest.raises(ValueError):
        op.update_values(coo_tensor(torch, col, row, v2, n))
    # astype rebuilds from the kept triplets, on the device
    opc = op.astype(np.complex128)
    assert opc.dtype == np.complex128 and opc.ingest_info["from_device"] and opc.ingest_info["coo_entries"] == len(row)
    assert_same_operator(eu, ctx, opc, eu.MIOperator(cc.expected_csr(row, col, v2.astype(np.complex128), n), ctx), np.complex128, "astype %s" % pattern)


# ------------------------------------------------------------------ 6. bad input is an error, not a fault
def test_bad_triplets_are_refused_before_anything_indexes_by_them(eu):
    ctx = eu.Context()
    n = 5000
    A = c2_operator(n)
    A.sort_indices()
    row0, col0, vals0 = cc.split_triplets(A, 0.1, "exact", 3)
    b = np.random.default_rng(9).standard_normal(n)
    good = eu.MIOperator(A, ctx)
    w0 = np.array(eu.expv(0.5, good, b, m=20, ishermitian=False, opnorm=1.0))
    lib = eu._lib.load()
    keep = []

    def attempt(row, col, base=0, nnz=None, idx_bytes=None, loc=1, idx=np.int64, null_col=False):
        arrs = [eu.DeviceArray.from_host(np.ascontiguousarray(x, dtype=t), ctx) for x, t in ((row, idx), (col, idx), (np.ones(len(row)), np.float64))]
        keep.extend(arrs)
        h = C.c_void_p()
        rc = lib.expv_mi_op_create_coo_loc(ctx._h, 0, n, len(row) if nnz is None else nnz, arrs[0].ptr, None if null_col else arrs[1].ptr, arrs[2].ptr,
                                           np.dtype(idx).itemsize if idx_bytes is None else idx_bytes, base, loc, C.byref(h))
        with pytest.raises(eu.ExpvMIError) as ei:
            eu.api._check(rc, ctx._h)
        assert ei.value.code == ARGUMENT_ERROR and h.value is None, (ei.value, h.value)
        return str(ei.value)

    for name, which in (("row", 0), ("column", 1)):
        said = "op_create_coo: %s index out of range" % name
        for idx in (np.int32, np.int64):
            for pos, bad_value, base in ((1234, n, 0), (len(row0) - 2, -1, 0), (77, 0, 1)):
                rc_ = [row0 + base, col0 + base]
                rc_[which] = rc_[which].copy()
                rc_[which][pos] = bad_value
                msg = attempt(rc_[0], rc_[1], base=base, idx=idx)
                assert said in msg and "(first at position %d)" % pos in msg, msg
        two = [row0.copy(), col0.copy()]
        two[which][[4321, 99, 2500]] = n + 3
        assert said + " (first at position 99)" in attempt(two[0], two[1])
    assert "op_create_coo: idx_bytes must be 4 or 8" in attempt(row0, col0, idx_bytes=2)
    assert "op_create_coo: negative nnz" in attempt(row0, col0, nnz=-1)
    assert "op_create_coo: null row / col / vals" in attempt(row0, col0, null_col=True)
    assert "op_create_coo: bad location" in attempt(row0, col0, loc=7)
    assert lib.expv_mi_op_create_coo_loc(ctx._h, 0, n, 0, None, None, None, 8, 0, 1, None) == ARGUMENT_ERROR      # null output
    ctx.sync()
    w1 = np.array(eu.expv(0.5, good, b, m=20, ishermitian=False, opnorm=1.0))
    assert np.array_equal(w0, w1)
    # and the context still creates operators: one-based int32 triplets from the library's own allocations, Julia's layout
    arrs = [eu.DeviceArray.from_host(x, ctx) for x in ((row0 + 1).astype(np.int32), (col0 + 1).astype(np.int32), vals0)]
    h = C.c_void_p()
    eu._lib.check(lib.expv_mi_op_create_coo_loc(ctx._h, 0, n, len(row0), arrs[0].ptr, arrs[1].ptr, arrs[2].ptr, 4, 1, 1, C.byref(h)), ctx._h)
    ok = RawOp(eu, ctx, h)
    assert_same_operator(eu, ctx, ok, good, np.float64, "one-based int32 triplets through the C ABI")
    out = (C.c_int64 * 8)()
    assert lib.expv_mi_op_ingest_info(ok._h, out) == 0
    assert out[0] == 1 and out[1] == 4 * (n + 1 + A.nnz) and out[2] == 0 and out[6] == len(row0) and out[7] > 0


# ------------------------------------------------------------------ 7. determinism and the plan cache
def test_the_same_triplets_twice_give_the_same_bits_and_the_cached_plan(eu, torch):
    A = _shuffle(c2_operator(30_000), 21)
    A.sort_indices()
    n = A.shape[0]
    row, col, vals = cc.split_triplets(A, 0.3, "random", 13)
    ctx = eu.Context()
    eu.plan_cache(clear=True)
    b = np.random.default_rng(4).standard_normal(n)
    ops = [from_triplets(eu, torch, ctx, row, col, vals, n) for _ in range(2)]
    assert not ops[0].ingest_info["plan_cached"] and ops[1].ingest_info["plan_cached"]
    Hs = [np.array(eu.arnoldi(op, b, m=25, ishermitian=False, opnorm=1.0).getH()) for op in ops]
    assert np.all(np.isfinite(Hs[0])) and np.array_equal(Hs[0], Hs[1])
    assert ops[0].opnorm_inf == ops[1].opnorm_inf


# ------------------------------------------------------------------ 8. gputests.jl:41-58 as an uncoalesced device COO tensor
def test_reference_gpu_test_from_an_uncoalesced_coo_tensor(eu, torch):
    n = 1000
    A = sprand_gputests(n)
    rng = np.random.default_rng(0x0452)
    b = rng.random(n) + 1j * rng.random(n)
    row, col, vals = cc.split_triplets(A, 0.15, "exact", 2)
    At, bt = coo_tensor(torch, row, col, vals, n), torch.as_tensor(b).cuda()
    assert not At.is_coalesced() and At._nnz() > A.nnz
    w = eu.expv(0.1, At, bt)
    assert torch.is_tensor(w) and w.is_cuda and w.dtype == torch.complex128
    close(w.cpu().numpy(), ko.expv(0.1, A, b), TOL, "gputests.jl:41-58 expv, A an uncoalesced device COO tensor, vs oracle")
    ts = np.linspace(0, 1, 300)
    E = eu.expv_timestep(ts.copy(), At, bt)
    assert torch.is_tensor(E) and E.is_cuda
    close(E.cpu().numpy(), ko.expv_timestep(ts.copy(), A, b), TOL, "gputests.jl:41-58 expv_timestep 300 snapshots, COO tensor, vs oracle")
    close(eu.phiv(0.2, At, bt, 2, m=20).cpu().numpy(), ko.phiv(0.2, A, b, 2, m=20), 1e-11, "phiv(device COO tensor)")
    # what to_sparse_coo() of a CSR tensor gives becomes the operator the CSR tensor gives; the plain constructor keeps refusing it
    Ac = to_torch_sparse(torch, A, np.int64)
    ctx = eu.Context()
    assert_same_operator(eu, ctx, eu.MIOperator.from_coo(Ac.to_sparse_coo(), ctx=ctx), eu.MIOperator(Ac, ctx), np.complex128, "to_sparse_coo()")
    with pytest.raises(TypeError, match="from_coo"):
        eu.MIOperator(Ac.to_sparse_coo(), ctx)
    # a CPU COO tensor is staged and takes the same path
    assert_same_operator(eu, ctx, eu.MIOperator.from_coo(At.cpu(), ctx=ctx), eu.MIOperator.from_coo(At, ctx=ctx), np.complex128, "CPU COO tensor")
    Ar = c2_operator(4000)
    br = rng.standard_normal(4000)
    rr, rc, rv = cc.split_triplets(Ar, 0.15, "exact", 3)
    wk, sk = eu.kiops(1.0, coo_tensor(torch, rr, rc, rv, 4000), br, ishermitian=False)
    wko, sko = ko.kiops(1.0, Ar, br, ishermitian=False)
    assert tuple(sk) == tuple(sko), (sk, sko)
    close(wk, wko, 1e-10, "kiops(device COO tensor)")
