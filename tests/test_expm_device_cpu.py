"""exponential!(A) for a dense matrix on the device and the product kernel behind it (expv_mi_expm / expv_mi_gemm), the part that
needs no GPU: the prototypes (header, library, ctypes table, Python API, Julia shim), the build list, the rule that there is no CPU
fallback, and the argument checks that come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import expv_mi_loader
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
