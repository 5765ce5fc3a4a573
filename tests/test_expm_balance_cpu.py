"""The balanced dense device exponential (expv_mi_expm_balanced / expv_mi_gebal / expv_mi_host_gebal), the part that needs no GPU:
the numpy restatement of the balancing (tests/balance_cases.py) against the oracle and against the host routine, the margins of
its decisions, the prototypes through every layer, and what balancing is worth on badly scaled matrices -- the same arithmetic as
the device's, on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import expv_mi_loader
from oracle import krylov_oracle as ko
from tests import balance_cases as bc
from tests import dense_cases as dc
from tests import test_abi_cpu as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"expv_mi_expm_balanced": 7, "expv_mi_gebal": 9, "expv_mi_host_gebal": 7}
ARGUMENT_ERROR = 2
F64, C64, F32, C32 = 0, 1, 2, 3
HOST, DEVICE = 0, 1
TOL = {"float64": 1e-11, "complex128": 1e-11, "float32": 1e-4, "complex64": 1e-4}
CPU_SIZES = (1, 2, 7, 33, 130)
# The host routine sums its norms in the element type's real type, the restatement (like the device) in fp64.  For the 32-bit types
# the two can differ by the rounding of a float32 sum of n squares (<= n eps32 relative, 1.6e-5 at n = 130) and of the factor 0.95
# (0.95f is 2.5e-8 off): the comparison with the HOST routine asks for decisions clear of that, a margin of 1e-4.
HOST32_MARGIN = 1e-4


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


def _cases(tname, margin=bc.MARGIN):
    out = []
    for n in CPU_SIZES:
        for E in (12, 20):
            out.append(("scaled n=%d E=%d" % (n, E), bc.scaled(tname, n, E, margin=margin)))
        for a, c in ((0, 3), (5, 0), (4, 6)):
            out.append(("isolated n=%d (%d, %d)" % (n, a, c), bc.isolated(tname, n, a, c, margin=margin)))
    for name in bc.DEGENERATE:
        out.append((name, bc.degenerate(name, tname)))
    return out


@pytest.mark.parametrize("tname", ["float64", "complex128"])
def test_the_restatement_is_the_oracle(tname):
    for name, case in _cases(tname):
        g = case["gebal"]
        W = np.array(case["A"], order="F", copy=True)
        ilo, ihi, scale = ko.gebal(W)
        assert (ilo, ihi) == (g["ilo"], g["ihi"]), name
        assert np.array_equal(scale, g["scale"]), name
        assert np.array_equal(W, g["A_bal"]), name
        # ... and unbalance is the oracle's inverse similarity
        X = np.random.default_rng(1).standard_normal(W.shape).astype(W.dtype)
        assert np.array_equal(bc.unbalance(X, ilo, ihi, scale), ko.gebak_similarity(X.copy(order="F"), ilo, ihi, scale)), name


@pytest.mark.parametrize("tname", bc.TYPES)
def test_the_restatement_is_the_host_routine(eu, tname):
    margin = HOST32_MARGIN if dc.real_type(tname) == np.float32 else bc.MARGIN
    for name, case in _cases(tname, margin):
        g = case["gebal"]
        assert g["margin"] >= margin
        B, ilo, ihi, scale = eu.host_gebal(case["A"])
        assert B.dtype == np.dtype(tname)
        assert (ilo, ihi) == (g["ilo"], g["ihi"]), name
        assert np.array_equal(scale, g["scale"]), name
        assert bc.same_bits(B, g["A_bal"]), name
        assert np.array_equal(case["A"], np.asarray(case["A"]))      # host_gebal works on a copy


@pytest.mark.parametrize("tname", bc.TYPES)
def test_every_decision_has_its_margin_and_no_case_is_left_out(tname):
    names = set()
    for name, case in _cases(tname):
        g = case["gebal"]
        names.add(name)
        assert g["margin"] >= bc.MARGIN, (name, g["margin"])
        assert g["sweeps"] < bc.BAL_MAX_SWEEPS
        assert np.all(np.log2(g["scale"][g["ilo"] - 1:g["ihi"]]) % 1 == 0)          # powers of two
        n = case["A"].shape[0]
        assert sorted(g["pos"]) == list(range(n))
    assert len(names) == len(CPU_SIZES) * 5 + len(bc.DEGENERATE)
    for n in (545, 1100):      # the sizes only the device tests run: their inputs are settled here too
        assert bc.scaled(tname, n, 20)["gebal"]["margin"] >= bc.MARGIN


@pytest.mark.parametrize("tname", bc.TYPES)
def test_balancing_recovers_d_up_to_a_common_factor(tname):
    for n in (7, 33, 130):
        for E in (12, 20):
            case = bc.scaled(tname, n, E)
            g = case["gebal"]
            assert (g["ilo"], g["ihi"]) == (1, n)
            off = bc.recovered_D(case)
            # the rows and columns of B have norms within a small factor of each other, and balancing stops within a factor 2 of
            # equal norms: every factor is D's within two binary orders of the common one
            assert off.max() - off.min() <= 4, (n, E, off.max() - off.min())
            assert np.log2(case["D"]).max() - np.log2(case["D"]).min() >= E
            assert g["norm1"] < 8.0 and dc.norm1_f64(case["A"]) > 2.0 ** (E - 2)


def test_the_degenerate_cases_take_the_paths_they_are_named_for():
    for tname in bc.TYPES:
        for name in ("permuted_triangular", "diagonal", "zero", "one", "negative_zeros"):
            g = bc.degenerate(name, tname)["gebal"]
            assert (g["ilo"], g["ihi"], g["sweeps"]) == (1, 1, 0), name
        z = bc.degenerate("zero_row_and_column", tname)
        assert (z["gebal"]["ilo"], z["gebal"]["ihi"]) == (1, 11) and z["gebal"]["pos"][11] == 4
        nz = bc.degenerate("negative_zeros", tname)["A"]
        as_nonzero = nz.copy()
        as_nonzero[(nz == 0) & np.signbit(np.real(nz))] = 1e-3       # were -0.0 to count as an entry, nothing would be isolated
        assert bc.gebal_restated(as_nonzero)["ihi"] == 8
        iso = bc.isolated(tname, 33, 4, 6)
        assert iso["blocks"] == (4, 23, 6) and (iso["gebal"]["ilo"], iso["gebal"]["ihi"]) == (5, 27)


def _header_protos():
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): abi._split_top(m.group(2).strip())
            for m in re.finditer(r"\bint\s+(expv_mi_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}


def test_the_three_prototypes_are_declared_exported_and_bound(eu):
    protos = _header_protos()
    L = eu.api.L
    lib = L.load()
    for name, nargs in NEW.items():
        assert name in protos and len(protos[name]) == nargs, name
        res, args = L.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert len(protos["expv_mi_expm"]) == 7                      # the unbalanced entry keeps its arguments
    for name in ("balance_", "host_gebal", "exponential", "exponential_"):
        assert name in eu.__all__ and callable(getattr(eu, name))
    import inspect
    for f in (eu.exponential, eu.exponential_):
        p = inspect.signature(f).parameters
        assert list(p)[:2] == ["A", "balance"] and p["balance"].default is False
    hdr = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    assert "EXPV_MI_K_COUNT = 11" in hdr and "AFTER balancing" in hdr
    engine_h = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "engine.h")).read()
    assert "dense_gebal_run" in engine_h


def test_the_julia_shim_has_the_new_methods():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert re.search(r"function ExponentialUtilities\.exponential!\(A::MIMatrix\{T\}, ::ExponentialUtilities\.ExpMethodHigham2005Base, cache = nothing\)", src)
    assert re.search(r"function balance!\(A::MIMatrix\{T\}\) where \{T <: MIScalar\}", src)
    # the two existing methods stay as written
    assert "function ExponentialUtilities.exponential!(A::MIMatrix{T}) where {T <: MIScalar}" in src
    assert ("ExponentialUtilities.exponential!(A::MIMatrix{T}, ::ExponentialUtilities.ExpMethodHigham2005, cache = nothing) where {T <: MIScalar} =\n"
            "    ExponentialUtilities.exponential!(A)") in src
    used = set(re.findall(r":(expv_mi_[a-z0-9_]+), lib", src))
    assert {"expv_mi_expm_balanced", "expv_mi_gebal"} <= used
    abi.test_julia_shim_calls_match_the_header()


def test_documents_name_the_entries():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "expv_mi_expm_balanced" in text and "expv_mi_gebal" in text, doc
    assert "expv_mi_host_gebal" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "expm_balance.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "expm_balance.py"))


def test_argument_checks_answer_without_a_device(eu):
    lib = eu.api.L.load()
    buf = np.zeros((4, 4), order="F")
    p = buf.ctypes.data
    info = (ctypes.c_int64 * 8)()
    ilo, ihi = ctypes.c_int64(-7), ctypes.c_int64(-7)
    scale = np.zeros(4)
    expm = lib.expv_mi_expm_balanced
    assert expm(None, F64, -1, p, 4, HOST, info) == ARGUMENT_ERROR
    assert expm(None, F64, 4, p, 3, HOST, info) == ARGUMENT_ERROR
    assert expm(None, F64, 4, None, 4, HOST, info) == ARGUMENT_ERROR
    assert expm(None, 9, 4, p, 4, HOST, info) == ARGUMENT_ERROR
    assert expm(None, F64, 4, p, 4, 5, info) == ARGUMENT_ERROR
    assert expm(None, F64, 0, None, 0, HOST, info) == 0 and expm(None, C32, 0, None, 0, DEVICE, None) == 0
    gebal = lib.expv_mi_gebal
    args = (ctypes.byref(ilo), ctypes.byref(ihi), scale.ctypes.data)
    assert gebal(None, F64, -1, p, 4, HOST, *args) == ARGUMENT_ERROR
    assert gebal(None, F64, 4, p, 3, HOST, *args) == ARGUMENT_ERROR
    assert gebal(None, F64, 4, None, 4, HOST, *args) == ARGUMENT_ERROR
    assert gebal(None, 9, 4, p, 4, HOST, *args) == ARGUMENT_ERROR
    assert gebal(None, F64, 4, p, 4, 5, *args) == ARGUMENT_ERROR
    assert gebal(None, F32, 0, None, 0, DEVICE, *args) == 0 and (ilo.value, ihi.value) == (1, 0)
    hg = lib.expv_mi_host_gebal
    assert hg(9, 4, p, 4, *args) == ARGUMENT_ERROR and hg(F64, 4, p, 3, *args) == ARGUMENT_ERROR and hg(F64, 4, None, 4, *args) == ARGUMENT_ERROR
    assert hg(F64, 0, None, 0, *args) == 0
    assert hg(F64, 4, p, 4, None, None, None) == 0               # every output is optional
    assert np.array_equal(buf, np.zeros((4, 4)))
    with pytest.raises(eu.DimensionMismatch):
        eu.balance_(np.zeros((3, 4)))
    with pytest.raises(TypeError, match="float32 / float64 / complex64 / complex128"):
        eu.balance_(np.eye(3, dtype=np.int64))
    with pytest.raises(eu.DimensionMismatch):
        eu.host_gebal(np.zeros((3, 4)))


# what balancing is worth, on the CPU in the element type: (type, n, E) of the table in DESIGN.md 4.1.2
TABLE = [("float64", 96, 12), ("float64", 130, 20), ("complex128", 96, 12), ("float32", 96, 12), ("float32", 130, 20), ("complex64", 130, 20)]


@pytest.mark.parametrize("tname,n,E", TABLE)
def test_unbalanced_misses_the_bar_and_balanced_meets_it(tname, n, E):
    case = bc.scaled(tname, n, E)
    A, truth = case["A"], case["truth"]
    with np.errstate(all="ignore"):
        U, _, uorder, us = dc.restatement(A)
        uerr = dc.rel_err(U, truth)
    B, g = bc.balanced_restatement(A)
    berr = dc.rel_err(B, truth)
    print("%s n=%d E=%d  |A|_1 %.1e -> %.2f  squarings %d -> %d  error %.1e -> %.1e" % (tname, n, E, dc.norm1_f64(A), g["norm1"], us, g["s"], uerr, berr))
    assert us >= 18 and g["s"] == 0 and g["norm1"] <= 2.0 * 1.0001
    assert not uerr < TOL[tname]              # (NaN where the squarings overflow)
    assert berr < TOL[tname] / 100


def test_the_inputs_tell_a_wrong_balancing_from_the_right_one():
    """Two of the mutations the device tests are meant to catch, applied to the restatement itself: leaving the diagonal out of c and r,
    and scanning the column phase from 1 instead of k.  On the inputs of the device tests they change ilo / ihi / scale, so a device
    routine with either fault cannot equal the (unmutated) restatement bit for bit."""
    for tname in bc.TYPES:
        diag = cols = 0
        for n in (7, 33, 130):
            cases = [bc.scaled(tname, n, E) for E in (12, 20)] + [bc.isolated(tname, n, a, c) for a, c in ((0, 3), (5, 0), (4, 6))]
            for case in cases:
                g = case["gebal"]
                same = lambda m: (m["ilo"], m["ihi"]) == (g["ilo"], g["ihi"]) and np.array_equal(m["scale"], g["scale"])
                diag += not same(bc.gebal_restated(case["A"], mutate="no_diagonal"))
                cols += not same(bc.gebal_restated(case["A"], mutate="columns_from_one"))
        assert diag >= 3, (tname, diag)
        assert cols == 6, (tname, cols)          # every `isolated` input with a > 0: (5, 0) and (4, 6) at the three sizes


@pytest.mark.parametrize("tname", ["float32", "complex64"])
def test_the_input_that_needs_fp64_sums(eu, tname):
    """the third mutation the device tests are meant to catch, float32 accumulation of the norms: tests/balance_cases.float32_sums_case
    is decided differently by float32 sums -- in numpy and in the host routine, which sums in the element type -- and by fp64 sums"""
    case = bc.float32_sums_case(tname)
    g = case["gebal"]
    assert 1e-9 <= g["margin"] <= 1e-8 and (g["ilo"], g["ihi"]) == (1, 3)
    assert list(g["scale"]) == [4.0, 1.0, 64.0]
    assert list(bc.gebal_restated(case["A"], mutate="float32_sums")["scale"]) == [2.0, 1.0, 32.0]
    assert list(eu.host_gebal(case["A"])[3]) == [2.0, 1.0, 32.0]
    row = case["A"][0, :].astype(np.complex128)
    assert float(np.sum(np.abs(row) ** 2)) == 64.0 + 2.0 ** -20 and np.float32(64.0) + np.float32(2.0 ** -20) == np.float32(64.0)
