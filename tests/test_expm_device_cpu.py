"""exponential!(A) for a dense matrix on the device and the product kernel behind it (expv_mi_expm / expv_mi_gemm), the part that
needs no GPU: the prototypes (header, library, ctypes table, Python API, Julia shim), the build list, the rule that there is no CPU
fallback, the argument checks that come before any device work, and the properties of the inputs of the device stress tests
(tests/dense_cases.py) that those tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import expv_mi_loader
from oracle import krylov_oracle as ko
from tests import dense_cases as dc
from tests import test_abi_cpu as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"expv_mi_expm": 7, "expv_mi_gemm": 15}
ARGUMENT_ERROR = 2          # EXPV_MI_ARGUMENT_ERROR
F64, C64, F32, C32 = 0, 1, 2, 3
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def _header_protos():
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(expv_mi_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        out[m.group(1)] = abi._split_top(m.group(2).strip())
    return out


def test_both_prototypes_are_declared_exported_and_bound(eu):
    protos = _header_protos()
    L = eu.api.L
    lib = L.load()
    for name, nargs in NEW.items():
        assert name in protos, name + " is not declared in include/expv_mi.h"
        assert len(protos[name]) == nargs, (name, protos[name])
        assert name in L.PROTOTYPES, name + " is missing from _lib.PROTOTYPES"
        res, args = L.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs
        fn = getattr(lib, name)                       # exported by the library
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    # scalars of the product are doubles, sizes 64-bit
    _, args = L.PROTOTYPES["expv_mi_gemm"]
    assert [args[i] for i in (5, 6, 11, 12)] == [ctypes.c_double] * 4
    assert [args[i] for i in (2, 3, 4, 8, 10, 14)] == [ctypes.c_int64] * 6
    for name in ("exponential", "exponential_", "mul_"):
        assert name in eu.__all__ and callable(getattr(eu, name))


def test_the_new_source_is_built_and_keeps_to_the_rules_of_product_sources():
    build_py = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "build.py")).read()
    sources = re.search(r"SOURCES\s*=\s*\[(.*?)\]", build_py, flags=re.S).group(1)
    assert '"dense_dev.hip"' in sources
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "dense_dev.hip")).read()
    # the product kernel runs on the matrix cores for the 32-bit and the 64-bit element types
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in src and "__builtin_amdgcn_mfma_f64_16x16x4f64" in src
    assert len(re.findall(r"constexpr\s+int64_t\s+GEMM_BIG_TILE_MIN_OUTPUTS\b", src)) == 1      # ONE crossover constant, in this file
    assert "GEMM_BIG_TILE" not in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "kernels.h")).read()
    assert "asm" not in re.sub(r"//.*", "", src)          # plain C++ loads and stores only
    engine_h = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "engine.h")).read()
    assert "dense_expm_run" in engine_h and "dense_gemm_run" in engine_h
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    assert "EXPV_MI_K_COUNT = 11" in hdr                  # no new profiler id


def test_the_julia_shim_defines_the_methods_on_both_symbols():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert re.search(r"function ExponentialUtilities\.exponential!\(A::MIMatrix\{T\}\) where \{T <: MIScalar\}", src)
    assert re.search(r"ExponentialUtilities\.exponential!\(A::MIMatrix\{T\}, ::ExponentialUtilities\.ExpMethodHigham2005", src)
    assert re.search(r"function LinearAlgebra\.mul!\(C::MIMatrix\{T\}, A::MIMatrix\{T\}, B::MIMatrix\{T\}, α::Number, β::Number\)", src)
    used = set(re.findall(r":(expv_mi_[a-z0-9_]+), lib", src))
    assert set(NEW) <= used
    abi.test_julia_shim_calls_match_the_header()          # ... with the header's argument counts and kinds


def test_documents_name_the_entries():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "expv_mi_expm" in text, doc
    assert "expv_mi_gemm" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    assert "1382.4" in hdr                                # the uncapped scaling, stated where the entry is declared
    assert "expm_device.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_no_cpu_fallback(eu):
    """Without a device the dense exponential fails like every other product entry: HIPError from the context, never a host result."""
    A = np.eye(4)
    if not _no_gpu():      # (on a GPU box the same call simply works)
        assert np.allclose(eu.exponential_(A), np.e * np.eye(4), rtol=1e-13, atol=1e-15)
        return
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.exponential_(A)
    assert ei.value.kind == "HIPError"
    assert np.array_equal(A, np.eye(4))


def test_python_front_end_checks_before_any_device_work(eu):
    with pytest.raises(eu.DimensionMismatch):
        eu.exponential_(np.zeros((3, 4)))
    with pytest.raises(eu.DimensionMismatch):
        eu.exponential(np.zeros(5))
    for bad in (np.eye(3, dtype=np.int64), np.eye(3, dtype=np.int32), np.eye(3, dtype=bool)):
        with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
            eu.exponential_(bad)
    import torch
    with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
        eu.exponential_(torch.eye(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="GPU"):
        eu.exponential_(torch.eye(3))


def test_argument_checks_answer_without_a_device(eu):
    """Everything that can be refused from the arguments alone is refused before the context is touched: status 2 with a NULL context."""
    lib = eu.api.L.load()
    buf = np.zeros((4, 4), order="F")
    p = buf.ctypes.data
    info = (ctypes.c_int64 * 8)()
    expm = lib.expv_mi_expm
    assert expm(None, F64, -1, p, 4, HOST, info) == ARGUMENT_ERROR          # n < 0
    assert expm(None, F64, 4, p, 3, HOST, info) == ARGUMENT_ERROR           # lda < n
    assert expm(None, F64, 4, None, 4, HOST, info) == ARGUMENT_ERROR        # null pointer with n > 0
    assert expm(None, 9, 4, p, 4, HOST, info) == ARGUMENT_ERROR             # unknown dtype
    assert expm(None, F64, 4, p, 4, 5, info) == ARGUMENT_ERROR              # unknown loc
    assert expm(None, F64, 0, None, 0, HOST, info) == 0                     # n = 0: nothing to do
    assert expm(None, C32, 0, None, 0, DEVICE, None) == 0
    assert np.array_equal(buf, np.zeros((4, 4)))
    gemm = lib.expv_mi_gemm
    assert gemm(None, F64, -1, 4, 4, 1.0, 0.0, p, 4, p, 4, 0.0, 0.0, p, 4) == ARGUMENT_ERROR
    assert gemm(None, F64, 4, 4, 4, 1.0, 0.0, p, 3, p, 4, 0.0, 0.0, p, 4) == ARGUMENT_ERROR      # lda < m
    assert gemm(None, F64, 4, 4, 4, 1.0, 0.0, p, 4, p, 4, 0.0, 0.0, None, 4) == ARGUMENT_ERROR   # null C
    assert gemm(None, 7, 4, 4, 4, 1.0, 0.0, p, 4, p, 4, 0.0, 0.0, p, 4) == ARGUMENT_ERROR
    assert gemm(None, F64, 4, 4, 4, 1.0, 0.5, p, 4, p, 4, 0.0, 0.0, p, 4) == ARGUMENT_ERROR      # imaginary scalar, real type
    assert gemm(None, F32, 4, 4, 4, 1.0, 0.0, p, 4, p, 4, 0.0, -2.0, p, 4) == ARGUMENT_ERROR
    assert gemm(None, C64, 0, 4, 4, 1.0, 0.5, p, 4, p, 4, 0.0, 0.0, p, 4) == 0                   # empty C


# --------------------------------------------------------------------------------------------- inputs of the device stress tests
# (tests/dense_cases.py: what tests/test_gpu_expm_device_stress.py relies on, checked here without a device)

SKEW_CPU_CASES = [(t, n, 6) for n in (130, 545) for t in ("float64", "complex128", "float32", "complex64")] + [("float64", 1090, 7)]


@pytest.mark.parametrize("tname,n,k", SKEW_CPU_CASES)
def test_scattered_skew_blocks_pivot_with_fill_and_have_a_block_reference(tname, n, k):
    c = dc.skew_case(tname, n, k, 5.0)
    A, T = c["A"], np.dtype(tname)
    assert A.dtype == T and A.flags.f_contiguous and not A.flags.writeable
    eps = float(np.finfo(T).eps)
    colsums = np.abs(A.astype(np.complex128)).sum(axis=0)
    assert colsums.max() <= 5.0 * (1 + 8 * eps) and abs(c["norm1"] - 5.0) <= 5.0 * 8 * eps      # n does not push the norm up
    assert (c["order"], c["s"]) == (13, 0)
    if n == 130:
        whole = sl.expm(A.astype(np.complex128))
        assert dc.rel_err(whole, c["ref"]) < 1e-12
        assert np.linalg.norm(c["ref"].conj().T @ c["ref"] - np.eye(n)) < 1e-5 * n ** 0.5             # unitary (A rounded to T)
    st = c["stats"]
    print(tname, n, st, "restatement %.2e gap %.2e" % (c["restated_err"], c["gap"]))
    assert st["exchanges"] >= n / 25
    assert st["rows_twice"] >= 5
    assert st["leaving_panel"] >= 5
    if n == 1090:
        assert st["far"] >= 5                                         # pivots more than PANEL_THREADS rows below their column
    assert c["gap"] > 1000 * eps
    assert c["restated_err"] < (1e-14 if T.itemsize // (2 if T.kind == "c" else 1) == 8 else 1e-6)


def test_the_element_type_restatement_is_the_oracle_without_balancing():
    for n, k, norm1, bar in [(130, 6, 5.0, 1e-13), (130, 6, 0.5, 1e-13), (70, 5, 40.0, 1e-12)]:
        A, _ = dc.scattered_skew("float64", n, k, norm1, 7 + n)
        E, D, order, s = dc.restatement(A)
        want = ko.exponential_(A, balance=False)
        assert (order, s) == dc.expected_method(dc.norm1_f64(A))
        assert np.linalg.norm(E - want) / np.linalg.norm(want) < bar, (n, norm1)
    A, blocks = dc.scattered_skew("complex64", 70, 5, 5000.0, 3)
    E, _, order, s = dc.restatement(A)
    assert E.dtype == np.complex64 and (order, s) == (13, 10)          # ... and it goes past 8 squarings
    assert dc.rel_err(E, dc.block_reference(A, blocks)) < 1e-3


def test_expected_method_at_the_thresholds():
    up = lambda x: float(np.nextafter(x, np.inf))
    for thr, lo, hi in zip(dc.ORDER_THRESHOLDS, (3, 5, 7, 9), (5, 7, 9, 13)):
        assert dc.expected_method(thr) == (lo, 0) and dc.expected_method(up(thr)) == (hi, 0)
    assert dc.expected_method(5.4) == (13, 0) and dc.expected_method(up(5.4)) == (13, 1)
    assert dc.expected_method(10.8) == (13, 1) and dc.expected_method(up(10.8)) == (13, 2)
    assert dc.expected_method(5000.0) == (13, 10) and dc.expected_method(30000.0) == (13, 13)


@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("tname", ["float64", "complex128", "float32", "complex64"])
def test_threshold_matrices_have_exactly_the_intended_norm(tname, n):
    T = np.dtype(tname)
    R = dc.real_type(T).type
    for thr in dc.ORDER_THRESHOLDS + (5.4, 10.8):
        for v in (R(thr), np.nextafter(R(thr), R(np.inf)), np.nextafter(R(thr), R(0))):
            for imaginary in ((False, True) if T.kind == "c" else (False,)):
                A = dc.threshold_matrix(T, n, v, imaginary)
                assert A.dtype == T and A.shape == (n, n)
                if T.kind == "c":
                    assert np.all((A.real == 0) | (A.imag == 0))
                    assert np.count_nonzero(A.imag if imaginary else A.real) > 0
                sums = np.sort(np.abs(A.astype(np.complex128)).sum(axis=0))
                assert sums[-1] == float(v) == dc.norm1_f64(A)           # bit for bit, in double precision
                assert sums[-2] < float(v) / 64
                assert np.count_nonzero(A[:, n // 2]) == 1 and A[n // 2, n // 2] == 0
    if T.itemsize // (2 if T.kind == "c" else 1) == 8:
        assert float(R(0.25)) == 0.25 and float(R(2.1)) == 2.1


@pytest.mark.parametrize("seed", [2, 3, 5])
def test_the_fp64_norm_column_sums_above_a_quarter_only_in_double(seed):
    A, j = dc.fp64_norm_matrix(300, seed)
    assert A.dtype == np.float32 and A.shape == (300, 300)
    c = A[:, j]
    assert np.all(c > 0)
    s64 = float(np.sum(c.astype(np.float64)))
    assert 0.25 < s64 <= 0.25 + 2e-10
    f32 = dc.f32_sums(c)
    print(seed, "fp64 sum - 0.25 = %.3e" % (s64 - 0.25), f32)
    for name, v in f32.items():
        assert v <= 0.25, name
    others = np.delete(A.astype(np.float64).sum(axis=0), j)
    assert np.all(np.abs(others - 0.1) < 1e-6)
    assert dc.expected_method(dc.norm1_f64(A)) == (7, 0) and dc.expected_method(max(f32.values())) == (5, 0)
    assert seed != dc.FP64_NORM_SEED or np.array_equal(dc.fp64_norm_matrix()[0], A)


def test_the_wide_product_and_its_bound():
    rng = np.random.default_rng(5)
    for T in (np.float32, np.complex64, np.float64, np.complex128):
        A, B, C0 = (rng.integers(-3, 4, s).astype(T) for s in ((7, 9), (9, 5), (7, 5)))
        got, mag = dc.wide_product(-1, A, B, 1, C0)
        assert np.array_equal(got.astype(T), C0 - A @ B)
        assert np.array_equal(mag, np.abs(A) @ np.abs(B) + np.abs(C0))
        assert got.dtype.itemsize > np.dtype(T).itemsize
    u32 = 2.0 ** -24
    assert dc.product_gamma(np.float32, 1000) == 1002 * u32 and dc.product_gamma(np.float64, 129) == 131 * 2.0 ** -53
    assert abs(dc.product_gamma(np.complex64, 129) - 2 * 2 ** 0.5 * 133 * u32) < 1e-20


@pytest.mark.parametrize("n", [130, 1090])
@pytest.mark.parametrize("tname", ["float64", "complex128", "float32", "complex64"])
def test_tied_hub_blocks_exchange_twice_per_block_only_if_the_first_maximum_is_taken(tname, n):
    c = dc.tied_case(tname, n)
    A, blocks, T = c["A"], c["blocks"], np.dtype(tname)
    assert len(blocks) == n // 3 and (c["order"], c["s"]) == (13, 0)
    assert np.array_equal(A, -A.conj().T)
    for h, l1, l2 in blocks:
        assert h < l1 < l2 and np.array_equal(A[l1, :], A[l2, :]) and np.count_nonzero(A[l1, :]) == 1 and A[l1, h] != 0
    if T.kind == "c":
        assert np.all(A.real == 0) and np.count_nonzero(A.imag) == 4 * len(blocks)
    if n == 1090:      # ties between rows that one thread of the panel kernel holds in different trips of its row loop, and across waves
        assert sum(1 for h, l1, l2 in blocks if l2 - h >= dc.PANEL_THREADS) >= 20
    assert sum(1 for h, l1, l2 in blocks if (l1 - h) // 64 != (l2 - h) // 64) >= len(blocks) // 3      # ... held by different waves
    D = c["D"]
    for h, l1, l2 in blocks[:10]:
        assert abs(D[l1, h] - D[l2, h]) <= 8 * np.finfo(T).eps * abs(D[l1, h]) and abs(D[l1, h]) > 3 * abs(D[h, h])
    first, last = c["first"], c["last"]
    print(tname, n, "first maximum:", first, "last maximum:", last, "restatement %.2e" % c["restated_err"])
    assert first[0] == 2 * len(blocks) and last[0] == len(blocks)          # (exchanges)
    assert first[1] == last[1] == len(blocks)                               # one tied column per block
    assert min(first[2], last[2]) > 0.1                                     # every other decision: by 10 % or more
    assert c["restated_err"] < (1e-14 if dc.real_type(T) == np.float64 else 1e-6)
