"""Host side of the truncated-Taylor exp(tA)b (expv_mi_expv_taylor): the ABI, the theta tables and the parameter choice.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import expv_mi_loader
from tests import expv_taylor_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("expv_mi_expv_taylor", "expv_mi_host_taylor_theta", "expv_mi_host_taylor_params")
BITS = {0: 53, 1: 24}


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


def test_prototypes_are_declared_exported_and_bound(eu):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "expv_mi.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    from exponentialutilities_jl_amd import _lib, build
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["expv_mi_expv_taylor"][1]) == 13
    for name in ("expv_taylor", "expv_taylor_", "host_taylor_theta", "host_taylor_params"):
        assert name in eu.__all__ and callable(getattr(eu, name)), name
    assert "expv_taylor.hip" in build.SOURCES
    # no new struct, profiler id or counter slot came with it
    assert re.search(r"EXPV_MI_K_COUNT\s*=\s*11\b", hdr) and "expv_mi_ctx_counters(expv_mi_ctx_t ctx, int64_t out[8])" in hdr


@pytest.mark.parametrize("precision", [0, 1])
def test_theta_tables(tables, precision):
    th, tol = tables[precision], 2.0 ** -BITS[precision]
    assert len(th) == 55 and all(a < b for a, b in zip(th, th[1:])), "strictly increasing"
    assert th[0] == 2 * tol
    for m in range(1, tc.M_MAX + 1):
        want = tc.theta_mp(m, BITS[precision])
        assert abs(th[m - 1] - want) <= 1e-12 * want, (m, th[m - 1], want)


def test_theta64_agrees_with_the_published_values(tables):
    # Al-Mohy & Higham 2011, table 3.1 (three digits; also scipy's _expm_multiply)
    for m, pub in ((2, 2.58e-8), (5, 2.4e-3), (10, 1.44e-1), (30, 3.54), (55, 9.9)):
        assert abs(tables[0][m - 1] - pub) <= 0.05 * pub, (m, tables[0][m - 1], pub)


@pytest.mark.parametrize("precision", [0, 1])
def test_params_equal_the_restatement(eu, tables, precision):
    th = tables[precision]
    alphas = [0.0] + list(np.logspace(-12, 5, 200))
    for v in th:
        alphas += [v, float(np.nextafter(v, 0.0)), float(np.nextafter(v, np.inf))]
    for a in alphas:
        assert eu.host_taylor_params(a, precision) == tc.params(a, th), a
    assert eu.host_taylor_params(0.0, precision) == (0, 1)
    for m in (1, 17, 55):      # at theta_m exactly one stage of at most m terms does
        mm, s = eu.host_taylor_params(th[m - 1], precision)
        assert s == 1 and mm <= m


def test_arguments_outside_the_domain_are_refused(eu):
    for bad in (lambda: eu.host_taylor_theta(1, 2), lambda: eu.host_taylor_theta(0, 0), lambda: eu.host_taylor_theta(56, 1),
                lambda: eu.host_taylor_params(1.0, 2), lambda: eu.host_taylor_params(float("nan"), 0),
                lambda: eu.host_taylor_params(float("inf"), 0), lambda: eu.host_taylor_params(-1.0, 1)):
        with pytest.raises(eu.ExpvMIError) as ei:
            bad()
        assert ei.value.kind == "ArgumentError"


def test_restatement_cap_on_the_applications_across_precisions(tables):
    """What the GPU test asks of the device -- |applications - restatement's| <= s -- holds between the restatement's own 64- and
    32-bit runs on one table: a stage stops at most one borderline term apart."""
    n = 257
    for mk, alpha0 in ((tc.laplacian, 40.0), (tc.penta, 40.0), (tc.random8, 40.0)):
        for T64, T32 in ((np.float64, np.float32), (np.complex128, np.complex64)):
            A, b = mk(n, T32), tc.vector(n, T32)
            t = tc.t_for(A, alpha0)
            mu, alpha, _ = tc.shift_norm(A, t)
            i64 = tc.restated(t, A.astype(T64), b.astype(T64), T64, alpha, tables[1], tc.TOL[1], mu)[1]
            i32 = tc.restated(t, A, b, T32, alpha, tables[1], tc.TOL[1], mu)[1]
            assert abs(i64["applications"] - i32["applications"]) <= i64["s"], (mk.__name__, T32, i64, i32)


def test_no_cpu_fallback_without_gpu(eu):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor(1.0, np.eye(4), np.ones(4))
    assert ei.value.kind == "HIPError"
