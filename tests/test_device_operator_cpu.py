"""Sparse operators from device arrays, the part that needs no GPU: the helper that takes a torch.sparse_csr / sparse_csc tensor
apart, the new prototypes (header, library, ctypes table, Julia shim), and the rule that product sources name no test
infrastructure."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests import test_abi_cpu as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"expv_mi_op_create_csr_loc": 11, "expv_mi_op_create_csc_loc": 11, "expv_mi_op_ingest_info": 2}


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def _matrix(T, n=40, seed=1):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.15, random_state=rng, dtype=np.float64)
    if np.dtype(T).kind == "c":
        A = A + 1j * sp.random(n, n, density=0.15, random_state=rng, dtype=np.float64)
    A = A.tocsr().astype(T)
    A.sort_indices()
    return A


@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("T", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_unpacking_a_sparse_tensor(eu, fmt, T, idx):
    A = _matrix(T)
    M = A if fmt == "csr" else A.tocsc()
    M.sort_indices()
    mk = torch.sparse_csr_tensor if fmt == "csr" else torch.sparse_csc_tensor
    t = mk(torch.as_tensor(M.indptr).to(idx), torch.as_tensor(M.indices).to(idx), torch.as_tensor(M.data), size=M.shape)
    assert eu.api._is_torch_sparse(t) and not eu.api._is_torch_sparse(torch.zeros(3, 3))
    f, ptr, ind, vals, shape = eu.api._unpack_torch_sparse(t)
    assert f == fmt and shape == M.shape
    assert ptr.dtype == idx and ind.dtype == idx and ptr.is_contiguous() and ind.is_contiguous() and vals.is_contiguous()
    assert vals.dtype == getattr(torch, np.dtype(T).name)
    assert np.array_equal(ptr.numpy(), M.indptr) and np.array_equal(ind.numpy(), M.indices) and np.array_equal(vals.numpy(), M.data)
    # a CPU tensor takes the scipy path: the same matrix, the same format
    S = eu.api._torch_sparse_to_scipy(t)
    assert S.format == fmt and S.dtype == np.dtype(T) and (S != M).nnz == 0


def test_unpacking_refuses_what_is_not_one_square_csr_or_csc_matrix(eu):
    A = _matrix(np.float64)
    t = torch.sparse_csr_tensor(torch.as_tensor(A.indptr), torch.as_tensor(A.indices), torch.as_tensor(A.data), size=A.shape)
    for other in (t.to_sparse_coo(), t.to_sparse_bsr((2, 2)), t.to_sparse_bsc((2, 2))):
        with pytest.raises(TypeError, match=r"torch\.sparse_csr or torch\.sparse_csc"):
            eu.api._unpack_torch_sparse(other)
    batched = torch.stack([t.to_dense(), t.to_dense()]).to_sparse_csr()
    assert batched.dim() == 3
    with pytest.raises(eu.DimensionMismatch, match="batch"):
        eu.api._unpack_torch_sparse(batched)
    R = sp.random(6, 9, density=0.4, random_state=np.random.default_rng(2), format="csr")
    rect = torch.sparse_csr_tensor(torch.as_tensor(R.indptr), torch.as_tensor(R.indices), torch.as_tensor(R.data), size=R.shape)
    with pytest.raises(eu.DimensionMismatch, match="square"):
        eu.api._unpack_torch_sparse(rect)
    ints = torch.sparse_csr_tensor(torch.as_tensor(A.indptr), torch.as_tensor(A.indices), torch.arange(A.nnz), size=A.shape)
    with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
        eu.api._unpack_torch_sparse(ints)


def test_new_prototypes_are_declared_exported_and_bound(eu):
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
        assert m, "%s is not declared in include/expv_mi.h" % name
        assert len(abi._split_top(m.group(1))) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported" % name
        res, args = eu._lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs, (name, args)
    # the two creators differ from the host-only ones by the stated nnz and the location
    for fmt in ("csr", "csc"):
        assert "int64_t nnz" in re.search(r"expv_mi_op_create_%s_loc\s*\(([^;]*?)\)" % fmt, hdr, flags=re.S).group(1)
        assert "int loc" in re.search(r"expv_mi_op_create_%s_loc\s*\(([^;]*?)\)" % fmt, hdr, flags=re.S).group(1)


def test_ingest_info_and_creators_answer_without_a_device(eu):
    """argument checks that come before any device work"""
    out = (ctypes.c_int64 * 8)()
    assert eu._lib.load().expv_mi_op_ingest_info(None, out) == 2


def test_julia_shim_has_the_device_array_constructor():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert re.search(r"function MIOperator\(rowptr::MIVector\{Ti\}, colval::MIVector\{Ti\}, nzval::MIVector\{T\}, n::Integer;\s*"
                     r"format::Symbol = :csr, index_base::Integer = 1\)", src)
    used = set(re.findall(r":(expv_mi_[a-z0-9_]+), lib", src))
    assert set(NEW) <= used, sorted(set(NEW) - used)
    abi.test_julia_shim_calls_match_the_header()          # every ccall, the new ones included: declared symbol, declared arity


def test_product_sources_name_no_test_infrastructure():
    abi.test_product_never_imports_the_oracle()
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_ingest.hip")).read()
    assert "op_ingest.hip" in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "build.py")).read()
    assert "tests/" not in src and "pytest" not in src
