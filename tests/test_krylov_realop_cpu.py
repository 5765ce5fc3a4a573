"""Mixed calls (a real operator with complex vectors) without a GPU: the new entry points exist in the built library and in the
ctypes layer, and the oracle -- the yardstick of tests/test_gpu_krylov_realop.py -- follows the reference's rule T =
promote_type(eltype(A), eltype(b)): a real matrix with a complex b gives what its complex cast gives."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import expv_mi_loader
from oracle import krylov_oracle as ko
from tests import krylov_realop_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("expv_mi_op_apply_complex", "expv_mi_expv_realop", "expv_mi_phiv_timestep_realop", "expv_mi_ctx_last_path")


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def test_new_symbols_are_exported_declared_and_bound(eu):
    from exponentialutilities_jl_amd import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "%s is not exported by the library" % s
        assert s in _lib.PROTOTYPES, "%s is not bound in _lib.PROTOTYPES" % s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), "%s is not declared in include/expv_mi.h" % s
    # the two existing entries of a mixed call take the same arguments as before
    assert len(_lib.PROTOTYPES["expv_mi_op_apply_complex"][1]) == len(_lib.PROTOTYPES["expv_mi_op_apply"][1])
    assert len(_lib.PROTOTYPES["expv_mi_phiv_timestep_realop"][1]) == len(_lib.PROTOTYPES["expv_mi_phiv_timestep"][1])
    assert len(_lib.PROTOTYPES["expv_mi_expv_realop"][1]) == len(_lib.PROTOTYPES["expv_mi_expv"][1]) - 1      # (no w_dtype: the operator's complex type)


def test_path_flag_of_a_mixed_call(eu):
    from exponentialutilities_jl_amd import _lib
    assert _lib.PATH_REAL_OPERATOR == 2048
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    assert re.search(r"EXPV_MI_PATH_REAL_OPERATOR\s*=\s*2048\b", hdr)
    assert "real_operator" not in _lib.PATH_FLAGS and all(v != 2048 for v in _lib.PATH_FLAGS.values())      # the "path" list keeps its members


def test_python_entries_take_keep_real(eu):
    import inspect
    for f in (eu.arnoldi_, eu.lanczos_, eu.phiv_timestep_):
        p = inspect.signature(f).parameters
        assert "keep_real" in p and p["keep_real"].default is False, f.__name__
    assert callable(eu.MIOperator.matvec_complex)


@pytest.mark.parametrize("herm", [False, True], ids=["arnoldi", "lanczos"])
def test_oracle_promotes_a_real_matrix_under_a_complex_b(herm):
    """the yardstick: identical H, V and w for a real CSR matrix and for its complex cast"""
    n, m = 300, 20
    A = kc.sym_sell(n) if herm else kc.sell5(n)
    b = kc.cvector(n)
    Kr = ko.arnoldi(A, b, m=m, ishermitian=herm)
    Kc = ko.arnoldi(A.astype(np.complex128), b, m=m, ishermitian=herm)
    assert Kr.m == Kc.m == m
    assert np.array_equal(Kr.getH(), Kc.getH()) and np.array_equal(Kr.getV(), Kc.getV())
    assert np.asarray(Kr.getV()).dtype == np.complex128
    if herm:
        assert np.asarray(Kr.getH()).dtype == np.float64      # a Hermitian H is kept in the real type
    t = -0.7j
    wr, wc = ko.expv(t, A, b, m=30, ishermitian=herm), ko.expv(t, A.astype(np.complex128), b, m=30, ishermitian=herm)
    assert np.array_equal(wr, wc)
    truth = sl.expm(t * kc.as_dense(A).astype(np.complex128)) @ b
    assert np.linalg.norm(wr - truth) / np.linalg.norm(truth) <= kc.TOL_TRUTH


def test_oracle_timestep_takes_the_mix():
    n = 300
    A, b = kc.sell5(n), kc.cvector(n)
    ts = np.linspace(0.1, 0.7, 7)
    U = ko.expv_timestep(ts, A, b, tol=1e-10)
    Uc = ko.expv_timestep(ts, A.astype(np.complex128), b, tol=1e-10)
    assert np.asarray(U).dtype == np.complex128 and np.array_equal(U, Uc)
    B = np.stack([kc.cvector(n, seed=3 + k) for k in range(3)], axis=1)
    P = ko.phiv_timestep(ts, A, B, tol=1e-10)
    assert np.array_equal(P, ko.phiv_timestep(ts, A.astype(np.complex128), B, tol=1e-10))


def test_mul_bound_is_the_stated_formula():
    """mul_bound is (k + 2) u (|A| |x|) per real component, with k the stored entries of the row (n for dense) and u = 2^-53 / 2^-24:
    checked on rows whose k, |A| and |x| are known by hand"""
    import scipy.sparse as sp
    assert kc.unit_roundoff(np.float64) == 2.0 ** -53 and kc.unit_roundoff(np.float32) == 2.0 ** -24
    A = sp.csr_matrix(np.array([[2.0, 0.0, -3.0], [0.0, 0.0, 0.0], [1.0, -1.0, 4.0]]))      # k = 2, 0, 3
    x = np.array([1.0 - 2.0j, 5.0 + 0.5j, -1.0 + 1.0j])
    for R, u in ((np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)):
        bre, bim = kc.mul_bound(A.astype(R), x, R)
        assert np.array_equal(bre, np.array([4 * u * (2 * 1 + 3 * 1), 2 * u * 0.0, 5 * u * (1 + 5 + 4)]))
        assert np.array_equal(bim, np.array([4 * u * (2 * 2 + 3 * 1), 2 * u * 0.0, 5 * u * (2 + 0.5 + 4)]))
        dre, dim = kc.mul_bound(A.toarray().astype(R), x, R)                                 # dense: k = n for every row
        assert np.array_equal(dre, np.array([5 * u * 5.0, 5 * u * 0.0, 5 * u * 10.0])) and np.array_equal(dim, np.array([5 * u * 7.0, 0.0, 5 * u * 6.5]))
    re, im = kc.mul_reference(A, x)                                                          # the reference product itself
    assert np.array_equal(re.astype(np.float64), [5.0, 0.0, -8.0]) and np.array_equal(im.astype(np.float64), [-7.0, 0.0, 1.5])
