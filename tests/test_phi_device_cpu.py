"""phi!(out, A, k) for a dense matrix on the device (expv_mi_phi), the part that needs no GPU: the CPU sides of the device tests
(tests/phi_cases.py) against each other, the prototype (header, library, ctypes table, Python API, Julia shim), and the argument
checks that come before any device work."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import expv_mi_loader
from tests import dense_cases as dc
from tests import phi_cases as pc
from tests import test_abi_cpu as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGUMENT_ERROR = 2
F64, C64, F32, C32 = 0, 1, 2, 3
HOST, DEVICE = 0, 1
# the restatement's own worst errors over randn / skew / negsemi, n in {7, 33, 96}, norms up to 30 and at 1000 (measured on the CPU)
RESTATED_64, RESTATED_32 = 1e-14, 1e-5


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


# --------------------------------------------------------------------------------------------- the algorithm, on the CPU
def test_the_taylor_degree_follows_from_the_remainder_bound():
    """k! theta^(M+1) / (M+1+k)! (1 - theta / (M+2+k))^-1 at theta = 1: largest at k = 0, first below the unit roundoff at M = 18 / 10"""
    for T, M, u in (("float64", 18, 2.0 ** -53), ("complex128", 18, 2.0 ** -53), ("float32", 10, 2.0 ** -24), ("complex64", 10, 2.0 ** -24)):
        assert pc.degree(T) == M
        bound = lambda m, k: math.factorial(k) / math.factorial(m + 1 + k) / (1.0 - 1.0 / (m + 2 + k))
        assert bound(M, 0) <= u < bound(M - 1, 0)
        assert all(bound(M, k) <= bound(M, 0) for k in range(17))
    assert pc.products("float64", 4, 3) == 3 + 4 + 4 + 3 and pc.products("float32", 1, 0) == 3 + 2 + 1


def test_scalings_at_the_thresholds():
    up = lambda x: float(np.nextafter(x, np.inf))
    assert [pc.scalings(v) for v in (0.0, 0.3, 1.0, up(1.0), 2.0, up(2.0), 4.0, 5.0, 30.0, 1000.0, 1e6)] == [0, 0, 0, 1, 1, 2, 2, 3, 5, 10, 20]
    for v in (1.0, 1.5, 2.0, 3.0, 1000.0, 1024.0, up(1024.0), 1e300):
        s = pc.scalings(v)
        assert v * 2.0 ** -s <= 1.0 and (s == 0 or v * 2.0 ** -(s - 1) > 1.0)


@pytest.mark.parametrize("n", pc.PARITY_SIZES)
@pytest.mark.parametrize("tname", pc.TYPES)
def test_the_restatement_meets_the_parity_bars_on_the_device_tests_inputs(tname, n):
    worst = 0.0
    for family in pc.PARITY_FAMILIES:
        for norm1 in pc.PARITY_NORMS:
            A, ref = pc.case(tname, n, norm1, family)
            assert A.dtype == np.dtype(tname) and abs(pc.norm1_f64(A) - norm1) <= 4 * np.finfo(A.dtype).eps * norm1
            for k in pc.PARITY_ORDERS:
                phis, M, s = pc.restatement(A, k)
                assert (M, s) == (pc.degree(tname), pc.scalings(pc.norm1_f64(A)))
                for j in range(k + 1):
                    worst = max(worst, pc.rel_err(phis[j], ref[j]))
    print(tname, n, "restatement %.2e" % worst)
    assert worst < pc.PARITY_BAR[tname]
    assert worst < (RESTATED_64 if pc.real_type(tname) == np.float64 else RESTATED_32)


@pytest.mark.parametrize("tname", pc.TYPES)
def test_the_restatement_at_ten_scalings(tname):
    for family in ("skew", "negsemi"):
        A = pc.matrix(tname, 96, 1000.0, family)
        ref = pc.truth(A, 4)
        phis, _, s = pc.restatement(A, 4)
        err = max(pc.rel_err(phis[j], ref[j]) for j in range(5))
        print(tname, family, "s=%d restatement %.2e" % (s, err))
        assert s == 10 and err < pc.PARITY_BAR[tname]
        fewer, _, _ = pc.restatement(A, 4, drop_recovery=1)          # (what a missing recovery step does to the answer)
        assert pc.rel_err(fewer[1], ref[1]) > 1e-2


@pytest.mark.parametrize("tname", pc.TYPES)
def test_closed_forms(tname):
    T = np.dtype(tname)
    tol = 1e-14 if pc.real_type(T) == np.float64 else 1e-6
    # A = 0: I / j!, bit for bit
    phis, _, s = pc.restatement(np.zeros((6, 6), dtype=T), 4)
    assert s == 0 and all(np.array_equal(p, z) for p, z in zip(phis, pc.zero_truth(T, 6, 4)))
    # diagonal A: the scalar phi of every entry; the augmented truth agrees with it
    d = np.array([-3.0, -0.5, 0.0, 0.25, 2.0]) * (1j if T.kind == "c" else 1)
    A = np.diag(d).astype(T)
    want = pc.diagonal_truth(np.diag(A), 3)
    assert max(pc.rel_err(t, w) for t, w in zip(pc.truth(A, 3), want)) < 1e-14
    phis, _, s = pc.restatement(A, 3)
    assert s == 2 and max(pc.rel_err(p, w) for p, w in zip(phis, want)) < tol
    # A = a E_12 at 20 scalings
    A = pc.nilpotent(T, 5, 1e6)
    phis, _, s = pc.restatement(A, 4)
    want = pc.nilpotent_truth(A, 4)
    assert s == 20 and max(pc.rel_err(p, w) for p, w in zip(phis, want)) < tol
    assert max(pc.rel_err(t, w) for t, w in zip(pc.truth(pc.nilpotent(T, 5, 3.0), 4), pc.nilpotent_truth(pc.nilpotent(T, 5, 3.0), 4))) < 1e-14


def test_the_threshold_and_column_inputs_separate_the_two_norms():
    """the threshold matrices' infinity norm lies above their 1-norm, a column-heavy matrix's far below: scalings taken from the
    wrong norm show"""
    for T in pc.TYPES:
        R = pc.real_type(T).type
        for v in (R(1.0), R(2.0)):
            A = dc.threshold_matrix(T, 9, v)
            assert pc.norm1_f64(A) == float(v) and np.linalg.norm(A.astype(np.complex128), np.inf) > float(v)
            assert pc.scalings(float(np.linalg.norm(A.astype(np.complex128), np.inf))) == pc.scalings(float(v)) + 1
        A = pc.column_heavy(T, 40, 5.0)
        assert abs(pc.norm1_f64(A) - 5.0) < 1e-5 and pc.scalings(pc.norm1_f64(A)) == 3
        assert pc.scalings(float(np.linalg.norm(A.astype(np.complex128), np.inf))) == 0


# --------------------------------------------------------------------------------------------- the entry, without a device
def test_the_prototype_is_declared_exported_and_bound(eu):
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    assert "phi.jl:159-257" in hdr and "no NaN-fill convention" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+expv_mi_phi\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "expv_mi_phi is not declared in include/expv_mi.h"
    args = abi._split_top(m.group(1).strip())
    assert len(args) == 10 and "void *const *out" in args[6]
    L = eu.api.L
    assert "expv_mi_phi" in L.PROTOTYPES
    res, ctypes_args = L.PROTOTYPES["expv_mi_phi"]
    i64, vp, ci = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    assert res is ci and list(ctypes_args) == [vp, ci, i64, ci, vp, i64, vp, i64, ci, vp]
    fn = L.load().expv_mi_phi
    assert fn.restype is ci and len(fn.argtypes) == 10
    for name in ("phi", "phi_"):
        assert name in eu.__all__ and callable(getattr(eu, name))
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "dense_dev.hip")).read()
    assert len(re.findall(r"constexpr\s+int\s+PHI_MAX_K\s*=\s*16\b", src)) == 1
    assert "PHI_MAX_K" not in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "kernels.h")).read()


def test_the_julia_shim_defines_phi_on_device_matrices():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert re.search(r"function ExponentialUtilities\.phi!\(out::Vector\{<:MIMatrix\{T\}\}, A::MIMatrix\{T\}, k::Integer; caches = nothing, expmethod = nothing\)", src)
    assert re.search(r"ExponentialUtilities\.phi\(A::MIMatrix\{T\}, k::Integer", src)
    assert "expv_mi_phi" in set(re.findall(r":(expv_mi_[a-z0-9_]+), lib", src))
    abi.test_julia_shim_calls_match_the_header()


def test_documents_name_the_entry():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "expv_mi_phi" in open(os.path.join(ROOT, doc)).read(), doc
    assert "phi_device.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "phi_device.txt" in open(os.path.join(ROOT, "profiles", "README.md")).read()


def test_python_front_end_checks_before_any_device_work(eu):
    A = np.eye(3)
    for bad in (np.eye(3, dtype=np.int64), np.eye(3, dtype=bool)):
        with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
            eu.phi(bad, 1)
        with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
            eu.phi_([np.eye(3), np.eye(3)], bad, 1)
    with pytest.raises(TypeError):
        eu.phi_([np.eye(3, dtype=np.float32)] * 2, A, 1)                 # out of another element type
    with pytest.raises(eu.DimensionMismatch):
        eu.phi(np.zeros((3, 4)), 1)
    with pytest.raises(eu.DimensionMismatch):
        eu.phi_([np.eye(3), np.eye(3)], np.zeros((3, 4)), 1)
    with pytest.raises(eu.DimensionMismatch):
        eu.phi_([np.eye(3), np.eye(3)], A, 2)                            # two matrices for k + 1 = 3
    with pytest.raises(eu.DimensionMismatch):
        eu.phi_([np.eye(3), np.eye(4)], A, 1)
    with pytest.raises(eu.DimensionMismatch):
        eu.phi_(np.zeros((3, 7)), A, 1)                                  # a slab is n x (k + 1) n
    for k in (-1, 17, 1.5):
        with pytest.raises(ValueError, match="0..16"):
            eu.phi(A, k)
        with pytest.raises(ValueError, match="0..16"):
            eu.phi_(np.zeros((3, 6)), A, k)
    import torch
    with pytest.raises(TypeError, match="GPU"):
        eu.phi(torch.eye(3), 1)
    assert np.array_equal(A, np.eye(3))


def test_argument_checks_answer_without_a_device(eu):
    """status 2 with a NULL context for everything that can be refused from the arguments alone; `out` is never written"""
    phi = eu.api.L.load().expv_mi_phi
    A = np.zeros((4, 4), order="F")
    slab = np.full((4, 8), 7.0, order="F")
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    o = ptrs(slab.ctypes.data, slab.ctypes.data + 16 * 8)
    info = (ctypes.c_int64 * 8)()
    a = A.ctypes.data
    assert phi(None, F64, -1, 1, a, 4, o, 4, HOST, info) == ARGUMENT_ERROR          # n < 0
    assert phi(None, F64, 4, 1, a, 3, o, 4, HOST, info) == ARGUMENT_ERROR           # lda < n
    assert phi(None, F64, 4, 1, a, 4, o, 3, HOST, info) == ARGUMENT_ERROR           # ldo < n
    assert phi(None, F64, 4, -1, a, 4, o, 4, HOST, info) == ARGUMENT_ERROR          # k < 0
    assert phi(None, F64, 4, 17, a, 4, o, 4, HOST, info) == ARGUMENT_ERROR          # k > 16
    assert phi(None, 9, 4, 1, a, 4, o, 4, HOST, info) == ARGUMENT_ERROR             # unknown dtype
    assert phi(None, F64, 4, 1, a, 4, o, 4, 5, info) == ARGUMENT_ERROR              # unknown loc
    assert phi(None, F64, 4, 1, None, 4, o, 4, HOST, info) == ARGUMENT_ERROR        # null A
    assert phi(None, F64, 4, 1, a, 4, None, 4, HOST, info) == ARGUMENT_ERROR        # null out
    assert phi(None, F64, 4, 1, a, 4, ptrs(slab.ctypes.data, None), 4, HOST, info) == ARGUMENT_ERROR
    assert phi(None, F64, 4, 1, a, 4, ptrs(slab.ctypes.data, a + 8), 4, HOST, info) == ARGUMENT_ERROR                       # out[1] inside A
    assert phi(None, F64, 4, 1, a, 4, ptrs(slab.ctypes.data, slab.ctypes.data + 15 * 8), 4, HOST, info) == ARGUMENT_ERROR   # out[1] meets out[0]
    assert phi(None, F64, 4, 1, a, 4, o, 4, HOST, info) == ARGUMENT_ERROR           # ... and only then the null context
    assert phi(None, F64, 0, 3, None, 0, None, 0, HOST, info) == 0                  # n = 0: nothing to do
    assert phi(None, C32, 0, 0, None, 0, None, 0, DEVICE, None) == 0
    assert np.all(slab == 7.0) and np.all(A == 0.0)
