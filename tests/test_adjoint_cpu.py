"""The CPU restatement of the adjoint operator's definition (tests/adjoint_cases.py: adjoint_arrays) held against scipy, and the
argument checks of expv_mi_op_create_adjoint / expv_mi_op_adjoint_refresh that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import expv_mi_loader
from tests import adjoint_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGUMENT_ERROR = 2          # EXPV_MI_ARGUMENT_ERROR


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()._lib.load()


@pytest.mark.parametrize("conj", [False, True])
@pytest.mark.parametrize("T", ac.DTYPES)
@pytest.mark.parametrize("case", sorted(ac.CASES))
@pytest.mark.parametrize("n", [1, 2, 37, 300])
def test_restatement_is_scipys_transpose_with_stored_zeros_kept(n, case, T, conj):
    A = ac.CASES[case](n, T)
    assert A.has_sorted_indices and (n < 30 or (A.data == 0).any()), "the generator stores zeros"
    rp, ci, va, src = ac.adjoint_arrays(A.indptr, A.indices, A.data, conj)
    R = (A.conj().T if conj else A.T).tocsr()      # (a transposed view of the arrays: nothing is dropped)
    R.sort_indices()
    assert R.nnz == A.nnz
    assert np.array_equal(rp, R.indptr) and np.array_equal(ci, R.indices)
    assert va.dtype == A.dtype and np.array_equal(va, R.data)
    # the source map reproduces the values
    assert np.array_equal(va, np.conj(A.data[src]) if conj else A.data[src])
    assert sorted(src.tolist()) == list(range(A.nnz))


@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("case", sorted(ac.CASES))
def test_applying_it_twice_returns_the_input_arrays(case, T):
    A = ac.CASES[case](211, T)
    rp, ci, va, _ = ac.adjoint_arrays(A.indptr, A.indices, A.data, True)
    rp2, ci2, va2, _ = ac.adjoint_arrays(rp, ci, va, True)
    assert np.array_equal(rp2, A.indptr) and np.array_equal(ci2, A.indices) and np.array_equal(va2, A.data)


def test_repeated_coordinates_stay_separate_adjacent_and_in_entry_order():
    A = ac.upper(150, np.complex128)
    ip, ix, va = ac.with_repeat(A)
    assert len(ix) == A.nnz + 1
    rp, ci, v2, src = ac.adjoint_arrays(ip, ix, va, True)
    assert len(ci) == len(ix) and rp[-1] == len(ix)
    # the matrix is the adjoint of the input's (duplicates summed by scipy on both sides)
    import scipy.sparse as sp
    n = A.shape[0]
    got = sp.csr_matrix((v2, ci, rp), shape=(n, n)).toarray()
    assert np.array_equal(got, A.conj().T.toarray())
    # rows ascending (not strictly: the repeat), the two entries of the repeated coordinate adjacent and in input order
    rows = np.repeat(np.arange(n), np.diff(rp))
    key = rows.astype(np.int64) * n + ci
    assert np.all(np.diff(key) >= 0) and int(np.sum(np.diff(key) == 0)) == 1
    e = int(np.argmax(np.diff(key) == 0))
    assert src[e] < src[e + 1]


def test_create_adjoint_checks_its_arguments_without_a_device(lib):
    out = C.c_void_p(0x1234)
    # null output first (even with a null parent), then the null parent, whatever `how` says
    assert lib.expv_mi_op_create_adjoint(None, 2, None) == ARGUMENT_ERROR
    assert b"op_create_adjoint" in lib.expv_mi_last_error(None) and b"null output" in lib.expv_mi_last_error(None)
    assert lib.expv_mi_op_create_adjoint(None, 2, C.byref(out)) == ARGUMENT_ERROR
    assert b"op_create_adjoint" in lib.expv_mi_last_error(None) and b"parent" in lib.expv_mi_last_error(None)
    assert lib.expv_mi_op_create_adjoint(None, 7, C.byref(out)) == ARGUMENT_ERROR
    assert b"op_create_adjoint" in lib.expv_mi_last_error(None)
    assert out.value == 0x1234, "*out is untouched on failure"


def test_adjoint_refresh_refuses_null_handles(lib):
    assert lib.expv_mi_op_adjoint_refresh(None, None) == ARGUMENT_ERROR
    assert b"op_adjoint_refresh" in lib.expv_mi_last_error(None)
