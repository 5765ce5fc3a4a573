"""Host side of the block truncated-Taylor exp(tA)B (expv_mi_expv_taylor_block): the ABI and the front ends.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import expv_mi_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "expv_mi_expv_taylor_block"


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def test_prototype_is_declared_exported_and_bound(eu):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "expv_mi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    from exponentialutilities_jl_amd import _lib, build
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m, "not declared"
    assert len(m.group(1).split(",")) == 20
    assert hasattr(lib, NAME)
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 20
    assert len(_lib.PROTOTYPES["expv_mi_expv_taylor"][1]) == 13, "the single call's prototype is untouched"
    for name in ("expv_taylor_block", "expv_taylor_block_"):
        assert name in eu.__all__ and callable(getattr(eu, name)), name
    assert "expv_taylor_block.hip" in build.SOURCES and "expv_taylor.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "expv_taylor_block.hip"))
    # the layouts are named in the header and mirrored by the binding; no profiler id came with the kernels
    assert re.search(r"EXPV_MI_BLOCK_COL_MAJOR\s*=\s*0\b", hdr) and re.search(r"EXPV_MI_BLOCK_ROW_MAJOR\s*=\s*1\b", hdr)
    assert (_lib.BLOCK_COL_MAJOR, _lib.BLOCK_ROW_MAJOR) == (0, 1)
    assert re.search(r"EXPV_MI_K_COUNT\s*=\s*11\b", hdr)


def test_julia_shim_names_the_symbol_with_twenty_arguments():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    m = re.search(r"ccall\(\(:%s, lib\), Cint,\s*\(([^)]*)\)" % NAME, src)
    assert m, "the Julia shim does not call the block entry point"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 20
    assert re.search(r"expv_taylor!\(W::MIMatrix\{T\}, t::Number, A::MIOperator\{T\}, B::MIMatrix\{T\}", src)
    assert re.search(r"expv_taylor\(t::Number, A::MIOperator\{T\}, B::MIMatrix\{T\}", src)


def test_block_layout_of_strided_arrays(eu):
    """which (layout, ld) an array goes in with: decided on the host, no device needed"""
    lay = eu.api._block_layout
    COL, ROW = 0, 1
    assert lay(7, 3, 3, 1) == (ROW, 3) and lay(7, 3, 5, 1) == (ROW, 5)          # C order; rows of a wider C-ordered array
    assert lay(7, 3, 1, 7) == (COL, 7) and lay(7, 3, 1, 10) == (COL, 10)        # Fortran order; leading rows of a taller one
    assert lay(7, 1, 1, 1) == (ROW, 1) and lay(7, 1, 4, 1) == (ROW, 4)          # one column, contiguous / at a row stride
    assert lay(1, 3, 3, 1) == (ROW, 3)
    assert lay(7, 3, 2, 14) is None and lay(7, 3, 2, 1) is None                  # no unit stride; rows that overlap


def test_a_vector_is_not_a_block(eu):
    with pytest.raises(eu.api.DimensionMismatch):
        eu.expv_taylor_block(1.0, np.eye(4), np.ones(4))


def test_no_cpu_fallback_without_gpu(eu):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_block(1.0, np.eye(4), np.ones((4, 3)))
    assert ei.value.kind == "HIPError"
