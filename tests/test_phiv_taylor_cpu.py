"""Host side of the basis-free phiv_timestep (expv_mi_phiv_taylor): the ABI, the refusals that need no device, the theorem behind the
truth of the GPU tests, and the accuracy of the numpy restatement on every 64-bit case those tests run.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import expv_mi_loader
from oracle import krylov_oracle as ko
from tests import expv_taylor_cases as tc
from tests import phiv_taylor_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "expv_mi_phiv_taylor"
ARGUMENT_ERROR = 2


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


def test_symbol_is_declared_exported_and_bound(eu):
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    from exponentialutilities_jl_amd import _lib, build
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
    assert m, "not declared"
    assert len(m.group(1).split(",")) == 16
    assert hasattr(lib, NAME)
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 16
    for name in ("phiv_taylor", "phiv_taylor_"):
        assert name in eu.__all__ and callable(getattr(eu, name)), name
    assert "phiv_taylor.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "phiv_taylor.hip")).read()
    assert "PHIV_TAYLOR_PMAX = 8" in src
    assert "PHIV_TAYLOR_PMAX" not in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "kernels.h")).read()


def test_julia_shim_names_the_symbol_with_sixteen_arguments():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    m = re.search(r"ccall\(\(:%s, lib\), Cint,\s*\(([^)]*)\)" % NAME, src)
    assert m, "the Julia shim does not call the entry point"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 16
    assert re.search(r"phiv_taylor!\(w::MIVector\{T\}, t::Number, A::MIOperator\{T\}, B::MIMatrix\{T\}", src)
    assert re.search(r"phiv_taylor\(t::Number, A::MIOperator\{T\}, B::MIMatrix\{T\}", src)


def test_refusals_that_need_no_device(eu):
    """the ranges of ncols, layout and loc are checked before a handle is looked at: code and message through the C entry"""
    lib = eu._lib.load()
    buf = np.zeros(16)
    info, dinfo = (ctypes.c_int64 * 8)(*([7] * 8)), (ctypes.c_double * 8)(*([7.0] * 8))

    def call(ncols, layout, b_loc, w_loc):
        return lib.expv_mi_phiv_taylor(None, None, 1.0, 0.0, buf.ctypes.data, 4, ncols, layout, b_loc, buf.ctypes.data, w_loc, 0, 0, 0.0, info, dinfo)
    for ncols in (0, -3, 10):
        assert call(ncols, 0, 0, 0) == ARGUMENT_ERROR
        msg = lib.expv_mi_last_error(None).decode()
        assert msg.startswith("phiv_taylor: ncols = %d is outside 1 .. 9" % ncols), msg
        assert list(info) == [0] * 8 and list(dinfo) == [0.0] * 8
    assert call(3, 0, 5, 0) == ARGUMENT_ERROR and lib.expv_mi_last_error(None).decode() == "phiv_taylor: unknown loc"
    assert call(3, 0, 0, -1) == ARGUMENT_ERROR and lib.expv_mi_last_error(None).decode() == "phiv_taylor: unknown loc"
    assert call(3, 2, 0, 0) == ARGUMENT_ERROR
    assert lib.expv_mi_last_error(None).decode() == "phiv_taylor: unknown layout (0 = column-major, 1 = row-major)"
    assert call(3, 1, 0, 0) == ARGUMENT_ERROR and lib.expv_mi_last_error(None).decode() == "phiv_taylor: null context / operator"
    assert not buf.any()


def test_a_vector_is_not_a_block(eu):
    with pytest.raises(eu.api.DimensionMismatch):
        eu.phiv_taylor(1.0, np.eye(4), np.ones(4))


def test_no_cpu_fallback_without_gpu(eu):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.phiv_taylor(1.0, np.eye(4), np.ones((4, 3)))
    assert ei.value.kind == "HIPError"


@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_truth_is_the_sum_of_phi_functions(T):
    """Theorem 2.1 itself, independently of the series: the augmented exponential against sum_k t^k phi_k(tA) u_k with the oracle's
    dense phi functions, 12 x 12.  Both sides are exponentials of matrices of norm ~ 10 in the same arithmetic: 1e-12 is a hundred
    times what either loses and far below any mistake in the ordering of W or the powers of t."""
    n, p, t = 12, 3, 0.7
    A = tc.dense(n, T) * 4.0
    B = pc.block(n, p, T)
    B[:, 1:] *= n      # (forcing columns as large as u_0)
    want = np.zeros(n, dtype=tc.wide(T))
    for k in range(p + 1):
        w = np.zeros((n, max(k, 1) + 1), dtype=tc.wide(T), order="F")      # (the oracle's formula starts at k = 1; column 0 is phi_0)
        ko.phiv_dense_(w, (t * A).astype(tc.wide(T)), B[:, k].astype(tc.wide(T)), max(k, 1))
        want += t ** k * w[:, k]
    assert tc.relmax(pc.truth(t, A, B), want) <= 1e-12


def test_nu_is_an_exact_power_of_two():
    assert [pc.nu_of(w) for w in (0.0, 1.0, 0.75, 0.5, 1.5, 2.0, 3.0, 2.0 ** -40, 1.25 * 2.0 ** 30)] == \
        [1.0, 1.0, 1.0, 2.0, 0.5, 0.5, 0.25, 2.0 ** 40, 2.0 ** -31]


@pytest.mark.parametrize("T", [np.float64, np.complex128])
@pytest.mark.parametrize("kind", pc.OPERATORS)
def test_restatement_stays_below_64_eps_on_the_64_bit_gpu_cases(tables, kind, T):
    """every 64-bit case of tests/test_gpu_phiv_taylor.py (parity and only-u_p): the restatement in the element type against the
    truth, <= 64 eps in the relative max norm.  A case that loses this is replaced, not loosened."""
    worst = 0.0
    for n, p, only_last, ct in pc.parity_cases(T):
        A = pc.operator(kind, n, T)
        B = pc.block(n, p, T, only_last=only_last)
        t = pc.t_for(A, B, pc.alpha_for(kind, T), ct)
        F, _ = pc.restated(t, A, B, T, tables[0], tc.TOL[0])
        e = tc.relmax(F, pc.truth(t, A, B)) / tc.eps_of(T)
        worst = max(worst, e)
        assert e <= 64, "%s n=%d p=%d only_last=%s complex_t=%s: %.1f eps" % (kind, n, p, only_last, ct, e)
    print("[phiv_taylor] %s %s: worst restatement error %.1f eps" % (kind, np.dtype(T).name, worst))
