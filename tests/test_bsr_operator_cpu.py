"""Sparse operators from block-compressed arrays, the part that needs no GPU: the position contract restated in numpy
(tests/bsr_cases.py) against scipy, the helper that takes a torch.sparse_bsr / sparse_bsc tensor apart, the new prototype (header,
library, ctypes table, Julia shim) and the tile constant the GPU tests size their cases by."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests import bsr_cases as bc
from tests import test_abi_cpu as abi
from tests.limits import parse_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
NB = 19


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def _case(bd, T=np.float64, unsorted=True):
    """empty block rows at the start, in the middle and at the end; stored zeros; block rows in reverse order"""
    ptr, idx, vals = bc.with_empty_block_rows(NB, bd, T, seed=10 + bd)
    cnt = np.diff(ptr)
    assert cnt[0] == 0 and cnt[-1] == 0 and np.all(cnt[5:8] == 0) and cnt.max() >= 2
    vals[::3, 0, bd - 1] = 0                      # zeros inside stored blocks
    vals[1] = 0                                   # ... and a whole block of them
    if unsorted:
        ptr, idx, vals = bc.reverse_block_rows(ptr, idx, vals)
        assert np.any(np.diff(idx) < 0)
    return ptr, idx, vals


# ------------------------------------------------------------------ the contract against scipy
@pytest.mark.parametrize("bd", [1, 2, 3, 5])
def test_the_restatement_is_scipys_tocsr(bd):
    ptr, idx, vals = _case(bd)
    S = sp.bsr_matrix((vals, idx, ptr), shape=(NB * bd, NB * bd)).tocsr()
    sptr, sidx, sval = bc.expand(ptr, idx, vals, bd)
    assert np.array_equal(sptr, S.indptr) and np.array_equal(sidx, S.indices) and np.array_equal(sval, S.data)
    assert len(sval) == len(idx) * bd * bd and np.count_nonzero(sval == 0) >= bd * bd          # stored zeros kept
    if bd > 1:
        assert not S.has_sorted_indices                                                         # unsorted block rows kept
    # one-based arrays are the same matrix
    s1 = bc.expand(ptr + 1, idx + 1, vals, bd, index_base=1)
    assert all(np.array_equal(a, b) for a, b in zip(s1, (sptr, sidx, sval)))


@pytest.mark.parametrize("bd", [1, 2, 3, 5])
def test_column_major_blocks_give_the_same_arrays(bd):
    ptr, idx, vals = _case(bd)
    want = bc.expand(ptr, idx, vals, bd)
    got = bc.expand(ptr, idx, bc.as_block_order(vals, "col"), bd, block_order="col")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("order", ["row", "col"])
@pytest.mark.parametrize("bd", [1, 2, 3, 5])
def test_bsc_is_the_restatements_csc(bd, order):
    """BSC of A, taken from A.T as BSR with transposed blocks, expands to the CSC arrays of A"""
    ptr, idx, vals = _case(bd, unsorted=False)
    n = NB * bd
    A = sp.bsr_matrix((vals, idx, ptr), shape=(n, n))
    cptr, cidx, cvals = bc.bsc_of(ptr, idx, vals, bd)
    sptr, sidx, sval = bc.expand(cptr, cidx, bc.as_block_order(cvals, order), bd, block_order=order, compressed="cols")
    C = sp.csc_matrix((sval, sidx, sptr), shape=(n, n))
    assert C.nnz == len(idx) * bd * bd and np.array_equal(C.toarray(), A.toarray())
    # position by position: scipy's tocsr of the transpose (whose rows are A's columns)
    St = sp.bsr_matrix((cvals.transpose(0, 2, 1), cidx, cptr), shape=(n, n)).tocsr()
    assert np.array_equal(sptr, St.indptr) and np.array_equal(sidx, St.indices) and np.array_equal(sval, St.data)
    M = bc.scalar_matrix(cptr, cidx, cvals, bd, compressed="cols")
    assert M.format == "csc" and np.array_equal(M.toarray(), A.toarray())


def test_repeated_blocks_stay_repeated():
    ptr, idx = np.array([0, 3, 3, 4]), np.array([2, 0, 2, 1])
    vals = np.arange(4 * 4, dtype=np.float64).reshape(4, 2, 2)
    sptr, sidx, sval = bc.expand(ptr, idx, vals, 2)
    assert list(sptr) == [0, 6, 12, 12, 12, 14, 16] and list(sidx[:6]) == [4, 5, 0, 1, 4, 5] and list(sval[:6]) == [0, 1, 4, 5, 8, 9]
    S = sp.bsr_matrix((vals, idx, ptr), shape=(6, 6)).tocsr()
    assert np.array_equal(sidx, S.indices) and np.array_equal(sval, S.data)


# ------------------------------------------------------------------ torch.sparse_bsr / sparse_bsc tensors taken apart
def _tensor(ptr, idx, vals, bd, compressed, it):
    n = (len(ptr) - 1) * bd
    mk = torch.sparse_bsr_tensor if compressed == "rows" else torch.sparse_bsc_tensor
    return mk(torch.as_tensor(ptr).to(it), torch.as_tensor(idx).to(it), torch.as_tensor(vals), size=(n, n))


@pytest.mark.parametrize("it", [torch.int32, torch.int64])
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("compressed", ["rows", "cols"])
def test_unpacking_a_block_sparse_tensor(eu, compressed, T, it):
    bd = 3
    ptr, idx, vals = bc.block_tridiagonal(7, bd, T)
    if compressed == "cols":
        ptr, idx, vals = bc.bsc_of(ptr, idx, vals, bd)
    t = _tensor(ptr, idx, vals, bd, compressed, it)
    assert eu.api._is_torch_sparse(t) and eu.api._is_torch_bsr(t)
    assert not eu.api._is_torch_bsr(t.to_dense().to_sparse_csr()) and not eu.api._is_torch_bsr(torch.zeros(3, 3))
    c, p, i, v, shape, b = eu.api._unpack_torch_bsr(t)
    assert (c, shape, b) == (compressed, (7 * bd, 7 * bd), bd)
    assert p.dtype == it and i.dtype == it and p.is_contiguous() and i.is_contiguous() and v.is_contiguous()
    assert v.dtype == getattr(torch, np.dtype(T).name) and tuple(v.shape) == (len(idx), bd, bd)
    assert np.array_equal(p.numpy(), ptr) and np.array_equal(i.numpy(), idx) and np.array_equal(v.numpy(), vals)
    assert v.data_ptr() == t.values().data_ptr()                                              # no copy
    # torch's own reading of the tensor is the restatement's matrix: row-major blocks in both layouts
    assert np.array_equal(t.to_dense().numpy(), bc.scalar_matrix(ptr, idx, vals, bd, "row", compressed).toarray())


def test_unpacking_refuses_what_is_not_one_square_matrix_of_square_blocks(eu):
    ptr, idx, vals = bc.block_tridiagonal(6, 2, np.float64)
    t = _tensor(ptr, idx, vals, 2, "rows", torch.int64)
    dense = t.to_dense()
    with pytest.raises(eu.DimensionMismatch, match="square blocks"):
        eu.api._unpack_torch_bsr(dense.to_sparse_bsr((2, 3)))
    with pytest.raises(eu.DimensionMismatch, match="batch"):
        eu.api._unpack_torch_bsr(torch.stack([dense, dense]).to_sparse_bsr((2, 2)))
    with pytest.raises(eu.DimensionMismatch, match="square"):
        eu.api._unpack_torch_bsr(dense[:, :8].to_sparse_bsr((2, 2)))
    ints = torch.sparse_bsr_tensor(torch.as_tensor(ptr), torch.as_tensor(idx), torch.ones(len(idx), 2, 2, dtype=torch.int64), size=(12, 12))
    with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
        eu.api._unpack_torch_bsr(ints)
    for other in (dense.to_sparse_csr(), dense.to_sparse_coo()):
        with pytest.raises(TypeError, match=r"torch\.sparse_bsr or torch\.sparse_bsc"):
            eu.api._unpack_torch_bsr(other)
    # the CSR / CSC helper keeps refusing the block layouts in its own words
    with pytest.raises(TypeError, match=r"torch\.sparse_csr or torch\.sparse_csc"):
        eu.api._unpack_torch_sparse(t)
    assert callable(eu.MIOperator.from_bsr)


def test_block_index_arrays_are_checked_before_any_device_work(eu):
    p, i = np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32)
    p2, i2 = eu.api._bsr_index_arrays(p, i)
    assert p2.dtype == np.int32 and p2.ctypes.data == p.ctypes.data
    pt, it = eu.api._bsr_index_arrays(torch.arange(5), torch.arange(4))
    assert isinstance(pt, np.ndarray) and pt.dtype == np.int64                                # CPU tensors: handed over as host arrays
    with pytest.raises(TypeError, match="int32 or int64"):
        eu.api._bsr_index_arrays(p, i.astype(np.int64))
    with pytest.raises(TypeError, match="both be torch tensors or both be arrays"):
        eu.api._bsr_index_arrays(torch.arange(5), i)
    with pytest.raises(eu.DimensionMismatch):
        eu.api._bsr_index_arrays(p.reshape(5, 1), i)


# ------------------------------------------------------------------ the boundary
def test_the_new_prototype_is_declared_exported_and_bound(eu):
    name, nargs = "expv_mi_op_create_bsr_loc", 13
    raw = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m, "%s is not declared in include/expv_mi.h" % name
    args = abi._split_top(m.group(1))
    assert len(args) == nargs and all(a in args for a in ("int64_t nnzb", "int block_dim", "int layout", "int loc", "const void *ptr"))
    enum = re.search(r"enum\s*\{([^}]*EXPV_MI_BSR_BLOCK_ROW_MAJOR[^}]*)\}", hdr).group(1)
    vals = dict(re.findall(r"(EXPV_MI_BSR_[A-Z_]+)\s*=\s*(\d+)", enum))
    assert vals == {"EXPV_MI_BSR_BLOCK_ROW_MAJOR": "0", "EXPV_MI_BSR_BLOCK_COL_MAJOR": "1", "EXPV_MI_BSR_COMPRESSED_COLS": "2"}
    L = eu._lib
    assert (L.BSR_BLOCK_ROW_MAJOR, L.BSR_BLOCK_COL_MAJOR, L.BSR_COMPRESSED_COLS) == (0, 1, 2)
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    assert hasattr(lib, name), "%s is not exported" % name
    res, bound = L.PROTOTYPES[name]
    assert res is ctypes.c_int and len(bound) == nargs
    # argument checks that come before any device work: a null output is an argument error, not a crash
    assert getattr(L.load(), name)(None, 0, 4, 1, 2, None, None, None, 4, 0, 0, 1, None) == 2


def test_julia_shim_takes_block_arrays():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert ":expv_mi_op_create_bsr_loc, lib" in src
    assert re.search(r"format in \(:bsr, :bsc\)", src) and "block_order" in src and "block_dim" in src
    abi.test_julia_shim_calls_match_the_header()
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "expv_mi_op_create_bsr_loc" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_tile_constant_is_readable_and_the_source_is_built():
    path = os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_bsr.hip")
    src = open(path).read()
    consts = parse_constants(src)
    assert consts["BSR_TILE"] % (4 * 256) == 0 and consts["BSR_TILE"] % 9 == 0      # whole trips; a whole number of 3 x 3 blocks
    assert "op_bsr.hip" in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "build.py")).read()
    assert "tests/" not in src and "pytest" not in src
