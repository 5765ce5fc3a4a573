"""Host side of exp(tA)b for a real operator with complex vectors (expv_mi_expv_taylor_realop): the ABI, the Julia binding, and the
accuracy of the restatement on the Float64-operator cases that the GPU test runs.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import expv_mi_loader
from tests import expv_taylor_cases as tc
from tests import expv_taylor_realop_cases as rc
from tests import taylor_dia_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "expv_mi_expv_taylor_realop"


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += {"(": 1, "{": 1, ")": -1, "}": -1}.get(ch, 0)
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def test_the_entry_is_declared_exported_and_bound_with_one_arity(eu):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "expv_mi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % NAME, hdr, flags=re.S)
    assert m, "include/expv_mi.h does not declare " + NAME
    cargs = _split_top(m.group(1))
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    from exponentialutilities_jl_amd import _lib, build
    assert hasattr(lib, NAME)
    assert len(cargs) == 14 and len(_lib.PROTOTYPES[NAME][1]) == len(cargs)
    assert [a.split()[-1].strip("*") for a in cargs][4:7] == ["b", "b_loc", "b_dtype"]
    for name in ("expv_taylor_realop", "expv_taylor_realop_"):
        assert name in eu.__all__ and callable(getattr(eu, name)), name
    assert "expv_taylor_realop.hip" in build.SOURCES
    # the existing single call is untouched, and no new struct, profiler id or counter slot came with the new one
    assert len(_lib.PROTOTYPES["expv_mi_expv_taylor"][1]) == 13
    assert re.search(r"EXPV_MI_K_COUNT\s*=\s*11\b", hdr) and "expv_mi_ctx_counters(expv_mi_ctx_t ctx, int64_t out[8])" in hdr


def test_the_julia_shim_binds_it():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    m = re.search(r"ccall\(\(:%s, lib\),\s*Cint,\s*\(" % NAME, src)
    assert m, "julia/MIKrylov.jl has no ccall of " + NAME
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
    assert len([a for a in _split_top(src[m.end(): i - 1]) if a]) == 14
    assert re.search(r"expv_taylor!\(w::MIVector\{Complex\{R\}\}, t::Number, A::MIOperator\{R\}", src)
    assert re.search(r"expv_taylor\(t::Number, A::MIOperator\{R\}, b::MIVector\{Complex\{R\}\}", src)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _restated_error(A, b, t, tables):
    Fr = rc.plan_and_restatement(A, b, t, tables)[4]
    dense = (A.toarray() if sp.issparse(A) else np.asarray(A)).astype(np.complex128)
    return tc.relmax(Fr, sl.expm(t * dense) @ b.astype(np.complex128))


@pytest.mark.parametrize("n", rc.SMALL_N)
@pytest.mark.parametrize("case", rc.SMALL_CASES, ids=rc.CASE_IDS)
def test_restatement_stays_below_64_eps_at_the_slice_boundaries(tables, case, n):
    """What lets the GPU test measure the device against 8 x max(restatement, eps): a real A run in complex128 keeps 64 eps (the
    Laplacian with t = -i tau at alpha = 10: 29 eps at worst; random8 on the ray at alpha = 40: 37 eps)."""
    _, mk, alpha, t_of = case
    A = mk(n, np.float64)
    e = _restated_error(A, rc.cvector(n, np.float64), t_of(A, alpha), tables)
    assert e <= 64 * tc.eps_of(np.complex128), "%s n = %d: %.1f eps" % (case[0], n, e / tc.eps_of(np.complex128))


def n1000_operators():
    n = 1000
    nx, ny = dc.PATCH_GRID
    return {"laplacian": (tc.laplacian(n, np.float64), rc.schroedinger_t, 10.0), "penta": (tc.penta(n, np.float64), rc.ray_t, 40.0),
            "random8": (tc.random8(n, np.float64), rc.ray_t, 40.0), "powerlaw": (tc.powerlaw(n, np.float64), rc.ray_t, 40.0),
            "dense": (tc.dense(n, np.float64), rc.ray_t, 40.0), "grid5": (dc.grid5(nx, ny + 1, np.float64, n=n), rc.schroedinger_t, 10.0),
            "shuffled_band": (tc.shuffled_band(n, np.float64)[0], rc.ray_t, 40.0)}


@pytest.mark.parametrize("name", ["laplacian", "penta", "random8", "powerlaw", "dense", "grid5", "shuffled_band"])
def test_restatement_stays_below_64_eps_on_every_operator_form(tables, name):
    A, t_of, alpha = n1000_operators()[name]
    e = _restated_error(A, rc.cvector(1000, np.float64), t_of(A, alpha), tables)
    assert e <= 64 * tc.eps_of(np.complex128), "%s: %.1f eps" % (name, e / tc.eps_of(np.complex128))


def test_restatement_with_a_real_b_and_an_imaginary_time(tables):
    n = 1000
    A = tc.penta(n, np.float64)
    e = _restated_error(A, tc.vector(n, np.float64), rc.schroedinger_t(A, 10.0), tables)
    assert e <= 64 * tc.eps_of(np.complex128), "%.1f eps" % (e / tc.eps_of(np.complex128))


def test_no_cpu_fallback_without_gpu(eu):
    import torch
    if torch.cuda.is_available():
        return      # (a GPU is present: tests/test_gpu_expv_taylor_realop.py has the call)
    with pytest.raises(eu.ExpvMIError) as ei:
        eu.expv_taylor_realop(1j, np.eye(4), np.ones(4))
    assert ei.value.kind == "HIPError"


def test_the_patch_grid_of_the_gpu_test_takes_the_ordering(eu):
    nx, ny = dc.PATCH_GRID
    for R in rc.REALS:
        perm, _, info = eu.host_patch_order(dc.grid5(nx, ny + 1, R, n=1000), R)
        assert info["patch_form"] and perm is not None, (R, info)
