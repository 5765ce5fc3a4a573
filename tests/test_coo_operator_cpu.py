"""Sparse operators from coordinate triplets, the part that needs no GPU: the CPU side of the contract (tests/coo_cases.py) against
itself and against scipy, the helper that takes a torch.sparse_coo tensor apart, the new prototype (header, library, ctypes
table, Julia shim) and the tile constant the GPU tests size their cases by."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests import coo_cases as cc
from tests import test_abi_cpu as abi
from tests.limits import parse_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def _matrix(T, n=60, seed=1):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.15, random_state=rng, dtype=np.float64)
    if np.dtype(T).kind == "c":
        A = A + 1j * sp.random(n, n, density=0.15, random_state=rng, dtype=np.float64)
    A = A.tocsr().astype(T)
    A.sort_indices()
    return A


# ------------------------------------------------------------------ the cases against themselves
@pytest.mark.parametrize("T", DTYPES)
def test_exact_splits_reproduce_the_original_bit_for_bit(T):
    A = _matrix(T)
    row, col, vals = cc.split_triplets(A, 0.4, "exact", 5)
    assert len(row) > A.nnz and vals.dtype == np.dtype(T)
    assert not np.array_equal(np.lexsort((col, row)), np.arange(len(row)))         # shuffled
    E = cc.expected_csr(row, col, vals, A.shape[0])
    assert np.array_equal(E.indptr, A.indptr) and np.array_equal(E.indices, A.indices)
    assert np.array_equal(E.data, A.data)


@pytest.mark.parametrize("T", DTYPES)
def test_random_parts_agree_with_scipy_to_rounding(T):
    A = _matrix(T)
    n = A.shape[0]
    row, col, vals = cc.split_triplets(A, 0.4, "random", 7)
    E = cc.expected_csr(row, col, vals, n)
    S = sp.coo_matrix((vals, (row, col)), shape=(n, n)).tocsr()
    S.sort_indices()
    assert np.array_equal(E.indptr, S.indptr) and np.array_equal(E.indices, S.indices)          # the pattern is scipy's
    # at most 3 parts per cell, each sum in its own order: |difference| <= 2 * 2 eps * sum |parts|
    mag = sp.coo_matrix((np.abs(vals).astype(np.float64), (row, col)), shape=(n, n)).tocsr()
    mag.sort_indices()
    eps = float(np.finfo(np.dtype(T).char.lower() if np.dtype(T).kind == "c" else T).eps)
    assert np.all(np.abs(E.data - S.data) <= 4 * eps * mag.data)


def test_expected_csr_keeps_empty_rows_and_stored_zeros():
    row, col, vals = np.array([4, 2, 2, 4, 2]), np.array([1, 3, 3, 0, 0]), np.array([1.0, 2.0, -2.0, 5.0, 7.0])
    E = cc.expected_csr(row, col, vals, 7)
    assert list(E.indptr) == [0, 0, 0, 2, 2, 4, 4, 4] and list(E.indices) == [0, 3, 0, 1]
    assert list(E.data) == [7.0, 0.0, 5.0, 1.0] and E.nnz == 4
    r, c, v = cc.random_triplets(37, 5000, np.float64, 3)
    assert len(r) == 5000 and cc.expected_csr(r, c, v, 37).nnz <= 37 * 37


# ------------------------------------------------------------------ torch.sparse_coo tensors taken apart
@pytest.mark.parametrize("coalesced", [True, False])
@pytest.mark.parametrize("T", DTYPES)
def test_unpacking_a_coo_tensor(eu, T, coalesced):
    A = _matrix(T)
    if coalesced:
        C = A.tocoo()
        t = torch.sparse_coo_tensor(torch.as_tensor(np.vstack([C.row, C.col]).astype(np.int64)), torch.as_tensor(C.data), size=A.shape).coalesce()
        row, col, vals = C.row, C.col, C.data
    else:
        row, col, vals = cc.split_triplets(A, 0.3, "exact", 9)
        t = torch.sparse_coo_tensor(torch.as_tensor(np.vstack([row, col])), torch.as_tensor(vals), size=A.shape)
        assert not t.is_coalesced()
    assert eu.api._is_torch_sparse(t) and eu.api._is_torch_coo(t) and not eu.api._is_torch_coo(t.to_sparse_csr())
    r, c, v, shape = eu.api._unpack_torch_coo(t)
    assert shape == A.shape and r.dtype == torch.int64 and c.dtype == torch.int64 and v.dtype == getattr(torch, np.dtype(T).name)
    assert r.is_contiguous() and c.is_contiguous() and v.is_contiguous()
    assert np.array_equal(r.numpy(), row) and np.array_equal(c.numpy(), col) and np.array_equal(v.numpy(), vals)
    assert r.data_ptr() == t._indices().data_ptr() and v.data_ptr() == t._values().data_ptr()          # no copy
    assert c.data_ptr() == r.data_ptr() + 8 * len(row)


def test_unpacking_refuses_what_is_not_one_square_scalar_coo_matrix(eu):
    A = _matrix(np.float64)
    C = A.tocoo()
    ind = torch.as_tensor(np.vstack([C.row, C.col]).astype(np.int64))
    hybrid = torch.sparse_coo_tensor(ind, torch.ones(C.nnz, 2, dtype=torch.float64), size=A.shape + (2,))
    with pytest.raises(eu.DimensionMismatch, match="dense dimensions"):
        eu.api._unpack_torch_coo(hybrid)
    batched = torch.sparse_coo_tensor(torch.as_tensor(np.vstack([np.zeros(C.nnz, dtype=np.int64), C.row, C.col])), torch.as_tensor(C.data), size=(2,) + A.shape)
    with pytest.raises(eu.DimensionMismatch, match="batch"):
        eu.api._unpack_torch_coo(batched)
    R = sp.random(6, 9, density=0.4, random_state=np.random.default_rng(2), format="coo")
    rect = torch.sparse_coo_tensor(torch.as_tensor(np.vstack([R.row, R.col]).astype(np.int64)), torch.as_tensor(R.data), size=R.shape)
    with pytest.raises(eu.DimensionMismatch, match="square"):
        eu.api._unpack_torch_coo(rect)
    ints = torch.sparse_coo_tensor(ind, torch.arange(C.nnz), size=A.shape)
    with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
        eu.api._unpack_torch_coo(ints)
    with pytest.raises(TypeError):
        eu.api._unpack_torch_coo(ints.to_dense().double().to_sparse_csr())
    # the CSR / CSC helper keeps refusing COO in its own words
    with pytest.raises(TypeError, match=r"torch\.sparse_csr or torch\.sparse_csc"):
        eu.api._unpack_torch_sparse(rect)


def test_triplet_index_arrays_are_checked_before_any_device_work(eu):
    r, c = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32)
    r2, c2 = eu.api._coo_index_arrays(r, c)
    assert r2.dtype == np.int32 and r2.ctypes.data == r.ctypes.data
    rt, ct = eu.api._coo_index_arrays(torch.arange(5), torch.arange(5))
    assert isinstance(rt, np.ndarray) and rt.dtype == np.int64            # CPU tensors: handed over as host arrays
    with pytest.raises(TypeError, match="int32 or int64"):
        eu.api._coo_index_arrays(r, c.astype(np.int64))
    with pytest.raises(TypeError, match="int32 or int64"):
        eu.api._coo_index_arrays(r.astype(np.float64), c.astype(np.float64))
    with pytest.raises(eu.DimensionMismatch):
        eu.api._coo_index_arrays(r, c[:4])
    assert callable(eu.MIOperator.from_coo)


# ------------------------------------------------------------------ the boundary
def test_the_new_prototype_is_declared_exported_and_bound(eu):
    name, nargs = "expv_mi_op_create_coo_loc", 11
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m, "%s is not declared in include/expv_mi.h" % name
    args = abi._split_top(m.group(1))
    assert len(args) == nargs and "int64_t nnz" in args and "int loc" in args and "const void *row" in args and "const void *col" in args
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    assert hasattr(lib, name), "%s is not exported" % name
    res, bound = eu._lib.PROTOTYPES[name]
    assert res is ctypes.c_int and len(bound) == nargs
    # argument checks that come before any device work: a null context is an argument error, not a crash
    assert getattr(eu._lib.load(), name)(None, 0, 1, 0, None, None, None, 4, 0, 1, None) != 0


def test_julia_shim_takes_triplets():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert ":expv_mi_op_create_coo_loc, lib" in src
    assert re.search(r"format in \(:csr, :csc, :coo\)", src)
    assert re.search(r"function MIOperator\(I::Vector\{Ti\}, J::Vector\{Ti\}, V::Vector\{T\}, n::Integer", src)
    abi.test_julia_shim_calls_match_the_header()
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "expv_mi_op_create_coo_loc" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_tile_constant_is_readable_and_the_source_is_built():
    path = os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_coo.hip")
    consts = parse_constants(open(path).read())
    assert consts["COO_TILE"] >= 256 and consts["COO_TILE"] % consts.get("BLOCK", 256) == 0
    assert "op_coo.hip" in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "build.py")).read()
    src = open(path).read()
    assert "tests/" not in src and "pytest" not in src
