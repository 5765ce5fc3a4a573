"""The CPU restatement of the linear-combination operator's definition (tests/lincomb_cases.py: lincomb_arrays) held against scipy,
the boundary of the two new entry points (header, library, ctypes binding, Julia shim) and the argument checks of
expv_mi_op_create_lincomb / expv_mi_op_lincomb_refresh that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import expv_mi_loader
from tests import lincomb_cases as lc
from tests import test_abi_cpu as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGUMENT_ERROR = 2          # EXPV_MI_ARGUMENT_ERROR


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def lib(eu):
    return eu._lib.load()


def exact_sum(terms, coefs, identity, n):
    """the dense matrix of the combination in complex128 (integer data: exact) and the union pattern as a boolean matrix"""
    S = np.zeros((n, n), dtype=np.complex128)
    P = np.zeros((n, n), dtype=bool)
    for t, c in zip(terms, coefs):
        M = lc.matrix(t)
        S += complex(c) * M.astype(np.complex128).toarray()
        rows = np.repeat(np.arange(n), np.diff(t[0]))
        P[rows, t[1]] = True
    if identity is not None:
        S += complex(identity) * np.eye(n)
        P |= np.eye(n, dtype=bool)
    return S, P


# integer coefficients (0 among them): every product and partial sum is an integer far below 2^24
INT_REAL = [2, -1, 1, -3, 1, 0, 2, -2]
INT_CPLX = [1 + 2j, -1, 1 - 1j, -3j, 2, 0, 1 + 1j, -2]


@pytest.mark.parametrize("T", lc.DTYPES)
@pytest.mark.parametrize("case", sorted(lc.CASES))
@pytest.mark.parametrize("n", [1, 2, 37, 300])
def test_restatement_is_scipys_sum_with_cancelled_and_zero_coefficient_entries_kept(n, case, T):
    terms = lc.CASES[case](n, T)
    K = len(terms)
    sets = [(INT_REAL[:K], None), (INT_REAL[:K], -2)]
    if np.dtype(T).kind == "c":
        sets += [(INT_CPLX[:K], None), (INT_CPLX[:K], 1 - 2j)]
    for coefs, identity in sets:
        rp, ci, va = lc.lincomb_arrays(terms, coefs, identity)
        S, P = exact_sum(terms, coefs, identity, n)
        assert va.dtype == np.dtype(T) and rp.dtype == np.int32 and ci.dtype == np.int32
        rows = np.repeat(np.arange(n), np.diff(rp))
        # the pattern: the union, row-major, strictly ascending -- decided by the patterns alone
        assert np.array_equal(np.flatnonzero(P.ravel()), rows.astype(np.int64) * n + ci), (case, n)
        got = np.zeros((n, n), dtype=np.complex128)
        got[rows, ci] = va
        assert np.array_equal(got, S), (case, n, coefs, identity)
    if n >= 37 and case in ("same_pattern", "zero_term"):
        # A - A keeps A's entries as stored zeros; a term with coefficient 0 keeps its pattern
        a = terms[0]
        rp, ci, va = lc.lincomb_arrays([a, a], [1, -1])
        assert np.array_equal(rp, a[0]) and np.array_equal(ci, a[1]) and not va.any() and len(va) > 0
        rp, ci, va = lc.lincomb_arrays(lc.CASES["two_bands"](n, T), [1, 0])
        assert len(ci) == 9 * n - 24, "both patterns are stored"


def test_repeated_coordinates_are_added_in_stored_order_and_the_accumulator_starts_as_the_first_contribution():
    T = np.float32
    big = np.float32(2.0 ** 24)
    # one row, the coordinate (0, 0) three times: (big + 1) + -big loses the 1 first; another stored order keeps it
    t1 = (np.array([0, 3], dtype=np.int32), np.zeros(3, dtype=np.int32), np.array([big, 1, -big], dtype=T))
    t2 = (np.array([0, 3], dtype=np.int32), np.zeros(3, dtype=np.int32), np.array([big, -big, 1], dtype=T))
    assert lc.lincomb_arrays([t1], [1.0])[2].tolist() == [0.0]
    assert lc.lincomb_arrays([t2], [1.0])[2].tolist() == [1.0]
    # term order: the same three contributions as three terms
    one = lambda v: (np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.array([v], dtype=T))      # noqa: E731
    assert lc.lincomb_arrays([one(big), one(1), one(-big)], [1, 1, 1])[2].tolist() == [0.0]
    assert lc.lincomb_arrays([one(big), one(-big), one(1)], [1, 1, 1])[2].tolist() == [1.0]
    # the identity comes last
    assert lc.lincomb_arrays([one(big), one(1)], [1, 1], identity=-float(big))[2].tolist() == [0.0]
    # -0 survives: the accumulator is the first contribution, not 0 + it
    z = lc.lincomb_arrays([one(-0.0)], [1.0])[2]
    assert z[0] == 0 and np.signbit(z[0])
    z = lc.lincomb_arrays([one(0.0)], [-1.0])[2]
    assert np.signbit(z[0])
    # a zero coefficient keeps its products: 0 * NaN is NaN
    assert np.isnan(lc.lincomb_arrays([one(1.0), one(np.nan)], [1.0, 0.0])[2][0])


def test_complex_products_are_four_rounded_products_and_a_real_coefficient_multiplies_each_component_once():
    T = np.complex64
    a = np.array([np.float32(1 / 3) + 1j * np.float32(1 / 7)], dtype=T)
    t = (np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), a)
    cr, ci = np.float32(0.1), np.float32(0.7)
    v = lc.lincomb_arrays([t], [complex(cr, ci)])[2][0]
    f = np.float32
    assert v.real == f(f(cr * a.real[0]) - f(ci * a.imag[0])) and v.imag == f(f(cr * a.imag[0]) + f(ci * a.real[0]))
    v = lc.lincomb_arrays([t], [float(cr)])[2][0]
    assert v.real == f(cr * a.real[0]) and v.imag == f(cr * a.imag[0])
    # a real coefficient never meets the other component: (-2) (1 + 0i) keeps the sign of the zero product, inf stays apart from NaN
    one = (np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.array([complex(np.inf, 1.0)], dtype=T))
    v = lc.lincomb_arrays([one], [-2.0])[2][0]
    assert v.real == -np.inf and v.imag == -2.0


# ------------------------------------------------------------------ the boundary
def test_the_new_prototypes_are_declared_exported_and_bound(eu):
    raw = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    L = eu._lib
    for name, nargs, must in (("expv_mi_op_create_lincomb", 5, ("int nterms", "const expv_mi_op_t *terms", "const double *coef", "int flags",
                                                                "expv_mi_op_t *op")),
                              ("expv_mi_op_lincomb_refresh", 4, ("expv_mi_op_t op", "int nterms", "const expv_mi_op_t *terms",
                                                                 "const double *coef"))):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
        assert m, "%s is not declared in include/expv_mi.h" % name
        args = [" ".join(a.split()) for a in abi._split_top(m.group(1))]
        assert len(args) == nargs and all(a in args for a in must), args
        assert hasattr(lib, name), "%s is not exported" % name
        res, bound = L.PROTOTYPES[name]
        assert res is C.c_int and len(bound) == nargs
    assert re.search(r"#define\s+EXPV_MI_LINCOMB_MAX_TERMS\s+8\b", hdr) and re.search(r"#define\s+EXPV_MI_LINCOMB_IDENTITY\s+1\b", hdr)
    assert (L.LINCOMB_MAX_TERMS, L.LINCOMB_IDENTITY) == (8, 1)
    flat = re.sub(r"\s*\n \*\s*", " ", raw)                        # (comment lines joined)
    for clause in ("never by a value or a coefficient", "An entry that cancels to zero stays stored", "the identity comes last",
                   "STARTS as the first contribution", "Nothing is fused and no floating-point atomic is used",
                   "4 (sum of nnz_k [+ n] + nnz + 1) bytes"):
        assert clause in flat, clause
    for f in ("lincomb", "recombine", "__add__", "__sub__", "__neg__", "__mul__", "__rmul__", "__truediv__"):
        assert callable(getattr(eu.MIOperator, f)), f
    # the cap lives in the new files and the public header, not in the header tests/limits.py reads
    csrc = os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc")
    assert "LINCOMB_MAX_TERMS = 8" in open(os.path.join(csrc, "op_lincomb.h")).read()
    assert "LINCOMB_MAX" not in open(os.path.join(csrc, "kernels.h")).read()
    src = open(os.path.join(csrc, "op_lincomb.hip")).read()
    assert "op_lincomb.hip" in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "build.py")).read()
    assert "fp contract(off)" in src and "atomicAdd" not in src and "tests/" not in src and "pytest" not in src


def test_julia_shim_combines_operators():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert ":expv_mi_op_create_lincomb, lib" in src and ":expv_mi_op_lincomb_refresh, lib" in src
    abi.test_julia_shim_calls_match_the_header()      # (argument counts and pointer / scalar kinds of every ccall, the two new ones among them)
    for method in (r"Base\.:\+\(A::MIOperator\{T\}, B::MIOperator\{T\}\)", r"Base\.:-\(A::MIOperator\{T\}, B::MIOperator\{T\}\)",
                   r"Base\.:-\(A::MIOperator\)", r"Base\.:\*\(c::Number, A::MIOperator\)", r"Base\.:\*\(A::MIOperator, c::Number\)",
                   r"Base\.:/\(A::MIOperator, c::Number\)", r"Base\.:\+\(A::MIOperator, J::UniformScaling\)",
                   r"Base\.:-\(A::MIOperator, J::UniformScaling\)", r"function lincomb\(terms::AbstractVector\{MIOperator\{T\}\}, coefs; identity = nothing\)",
                   r"function recombine!\(C::MIOperator\{T\}, coefs, terms"):
        assert re.search(method, src), method
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "expv_mi_op_create_lincomb" in open(os.path.join(ROOT, doc)).read(), doc


# ------------------------------------------------------------------ the checks that need no device
def test_create_lincomb_checks_its_arguments_without_a_device(lib):
    out = C.c_void_p(0x1234)
    coef = (C.c_double * 18)(*([1.0, 0.0] * 9))
    null_terms = (C.c_void_p * 8)()

    def refused(nterms, terms, co, flags, o, words):
        assert lib.expv_mi_op_create_lincomb(nterms, terms, co, flags, o) == ARGUMENT_ERROR
        msg = lib.expv_mi_last_error(None).decode()
        assert msg.startswith("op_create_lincomb: ") and all(w in msg for w in words), msg

    # in the order of the header: each call is wrong in everything that comes later as well
    refused(9, None, None, 6, None, ["null output"])
    refused(9, None, None, 6, C.byref(out), ["unknown flag bits"])
    refused(9, None, None, 1, C.byref(out), ["nterms"])
    refused(-1, None, None, 0, C.byref(out), ["nterms"])
    refused(0, None, None, 0, C.byref(out), ["nterms"])
    refused(0, None, coef, 1, C.byref(out), ["nterms", "identity"])      # the identity alone: nothing to take a context from
    refused(8, None, None, 1, C.byref(out), ["null coef"])
    refused(2, None, coef, 0, C.byref(out), ["null terms"])
    refused(8, null_terms, coef, 1, C.byref(out), ["null term"])
    assert out.value == 0x1234, "*op is untouched on failure"


def test_lincomb_refresh_refuses_null_handles(lib):
    assert lib.expv_mi_op_lincomb_refresh(None, 1, None, None) == ARGUMENT_ERROR
    assert b"op_lincomb_refresh" in lib.expv_mi_last_error(None)
