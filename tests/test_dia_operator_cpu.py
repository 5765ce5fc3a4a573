"""Sparse operators from stored diagonals, the part that needs no GPU: the position contract restated in numpy
(tests/dia_cases.py) against scipy, expv_mi_host_dia_pattern (the creator's pattern and its host-side checks) against the
restatement, the new prototypes (header, library, ctypes table, Julia shim), the tile constants the GPU tests size their cases
by, and the Python helpers that take a scipy dia matrix / a strided array apart."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests import dia_cases as dc
from tests import test_abi_cpu as abi
from tests.limits import parse_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGUMENT_ERROR = 2
OFFS = [-17, -1, 0, 1, 17]


@pytest.fixture(scope="module")
def eu():
    if not os.path.exists(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so")):
        expv_mi_loader.build()
    return expv_mi_loader.load()


# ------------------------------------------------------------------ the contract against scipy
@pytest.mark.parametrize("n", [1, 2, 18, 40])
def test_the_restatement_is_scipys_tocsr(n):
    offs = dc.scramble(OFFS + [40, -40, 3])
    diags = dc.random_diagonals(offs, n, np.float64)
    assert all(np.all(v != 0) for v in diags.values())
    data = dc.pack(diags, offs, n, "col", np.float64, ld=n, fill=0.0)          # (scipy reads the padding of a column-aligned row)
    S = sp.dia_matrix((data, offs), shape=(n, n)).tocsr()
    S.sort_indices()
    rp, ci, va, src = dc.expand(data, offs, n, "col")
    assert np.array_equal(rp, S.indptr) and np.array_equal(ci, S.indices) and np.array_equal(va, S.data)
    assert len(va) == dc.nnz_of(offs, n) and np.array_equal(rp, dc.rowptr_closed_form(offs, n))
    assert np.array_equal(dc.scalar_matrix(data, offs, n).toarray(), dc.dense_of(diags, n, np.float64))
    assert all(np.all(np.diff(ci[a:b]) > 0) for a, b in zip(rp[:-1], rp[1:]))          # rows sorted, no duplicates


def test_stored_zeros_stay_where_scipy_drops_them():
    n, offs = 12, [1, 0, -2]
    diags = dc.random_diagonals(offs, n, np.float64)
    diags[0][3] = 0.0
    diags[-2][:] = 0.0
    data = dc.pack(diags, offs, n, "col", np.float64, fill=0.0)
    S = sp.dia_matrix((data, offs), shape=(n, n)).tocsr()
    rp, ci, va, _ = dc.expand(data, offs, n)
    assert len(va) == dc.nnz_of(offs, n) == 3 * n - 3 and S.nnz == len(va) - 1 - (n - 2)
    assert np.count_nonzero(va == 0) == 1 + (n - 2)
    assert np.array_equal(dc.scalar_matrix(data, offs, n).toarray(), S.toarray())


@pytest.mark.parametrize("n", [1, 18, 33])
def test_alignments_and_offset_orders_give_the_same_arrays(n):
    offs = sorted(OFFS + [n - 1, -(n - 1), n, -n - 3] if n > 2 else [0, 1, -1])
    diags = dc.random_diagonals(offs, n, np.complex128)
    want = None
    for order in (offs, dc.scramble(offs), offs[::-1]):
        for align in dc.ALIGNS:
            for ld in (None, n + 5):
                data = dc.pack(diags, order, n, align, np.complex128, ld=ld)
                rp, ci, va, src = dc.expand(data, order, n, align)
                assert np.all(np.isfinite(va)) and len(np.unique(src)) == len(src)
                assert np.count_nonzero(np.isfinite(data)) == len(src)                  # every slot that is not read is NaN
                if want is None:
                    want = (rp, ci, va)
                assert all(np.array_equal(a, b) for a, b in zip((rp, ci, va), want)), (order, align, ld)
                assert np.array_equal(dc.nan_padding(data, order, n, align), data, equal_nan=True)


# ------------------------------------------------------------------ expv_mi_host_dia_pattern against the restatement
def _twin(eu, offsets, n, ld, align, arrays=True):
    return eu.host_dia_pattern(offsets, n, ld=ld, align=align, arrays=arrays)


CASES = [("n = 1", 1, [0]), ("n = 1, neighbours out of range", 1, [1, 0, -1]), ("dense", 33, list(range(-32, 33))),
         ("last superdiagonal", 33, [32]), ("last subdiagonal", 33, [-32]), ("out of range mixed in", 20, [25, -1, 0, -20, 20, 3, -400]),
         ("no diagonals", 7, []), ("only out of range", 7, [7, -7, 100]), ("scrambled", 300, [1, -17, 17, 0, -1])]


@pytest.mark.parametrize("align", dc.ALIGNS)
@pytest.mark.parametrize("what,n,offs", CASES, ids=[c[0] for c in CASES])
def test_host_dia_pattern_is_the_restatement(eu, what, n, offs, align):
    if what == "dense":
        offs = dc.scramble(offs, seed=4)
        assert len(offs) == 65
    for ld in (max(dc.min_ld(offs, n, align), 1), n + 5):
        rp, ci, _, src = dc.expand(None, offs, n, align, ld=ld)
        got = _twin(eu, offs, n, ld, align)
        inr = [k for k in offs if abs(k) < n]
        assert (got["nnz"], got["diagonals"]) == (dc.nnz_of(offs, n), len(inr)) == (len(ci), len(inr))
        assert (got["min_offset"], got["max_offset"]) == ((min(inr), max(inr)) if inr else (0, 0))
        assert np.array_equal(got["rowptr"], rp) and np.array_equal(got["colind"], ci) and np.array_equal(got["src"], src), what
        assert src.size == 0 or (src.min() >= 0 and src.max() < len(offs) * ld)
    if what == "dense":
        assert got["nnz"] == 33 * 33


# ------------------------------------------------------------------ every refusal, in order, with its message
def _refusal(eu, n, ndiag, offs, ld, align, out=True):
    lib = eu._lib.load()
    o = np.ascontiguousarray(offs, dtype=np.int64) if offs is not None else None
    res = (ctypes.c_int64 * 4)(-7, -7, -7, -7)
    rc = lib.expv_mi_host_dia_pattern(n, ndiag, o.ctypes.data if o is not None and o.size else None, ld, align, None, None, None,
                                      res if out else None)
    return rc, lib.expv_mi_last_error(None).decode(), list(res)


MESSAGES = ["null output", "unknown align", "n out of range for CSR32", "negative ndiag", "null offsets",
            "offset array contains duplicate values", "nnz exceeds CSR32", "ld is smaller than a diagonal's extent"]


def test_every_refusal_of_the_check_list_in_order(eu):
    big = 1 << 20
    wide = list(range(-1024, 1026))                      # 2050 offsets at n = 2^20: nnz = 2 148 530 175 > 2^31 - 1
    assert dc.nnz_of(wide, big) > 0x7fffffff
    # each attempt violates its own check AND every later one it can: the earlier check must answer
    attempts = [
        (dict(n=-1, ndiag=-1, offs=None, ld=-1, align=9, out=False), 0),
        (dict(n=-1, ndiag=-1, offs=None, ld=-1, align=3), 1),
        (dict(n=-1, ndiag=-1, offs=None, ld=-1, align=0), 2),
        (dict(n=1 << 31, ndiag=-1, offs=None, ld=-1, align=1), 2),
        (dict(n=5, ndiag=-1, offs=None, ld=-1, align=2), 3),
        (dict(n=5, ndiag=2, offs=None, ld=-1, align=0), 4),
        (dict(n=big, ndiag=len(wide) + 1, offs=wide + [7], ld=0, align=0), 5),
        (dict(n=5, ndiag=3, offs=[9, 1, 9], ld=0, align=0), 5),          # duplicates among out-of-range offsets too, as in scipy
        (dict(n=big, ndiag=len(wide), offs=wide, ld=0, align=1), 6),
        (dict(n=10, ndiag=2, offs=[0, 3], ld=9, align=0), 7),            # COL: n for k > 0
        (dict(n=10, ndiag=2, offs=[-4, -3], ld=6, align=0), 7),          # COL: n + k for k <= 0 (7 for k = -3)
        (dict(n=10, ndiag=2, offs=[3, 4], ld=6, align=1), 7),            # ROW: n - k for k >= 0
        (dict(n=10, ndiag=2, offs=[-3, 4], ld=9, align=1), 7),           # ROW: n for k < 0
        (dict(n=10, ndiag=2, offs=[-3, 4], ld=6, align=2), 7),           # START: n - |k|
    ]
    for kw, which in attempts:
        rc, msg, res = _refusal(eu, **kw)
        assert rc == ARGUMENT_ERROR and msg == "op_create_dia: " + MESSAGES[which], (kw["n"], kw["ndiag"], kw["ld"], kw["align"], msg)
        assert res == [-7] * 4, "out was written by a refused call"
    # ... and one short of each ld bound is accepted, with nothing allocated
    for kw in (dict(n=10, ndiag=2, offs=[-4, -3], ld=7, align=0), dict(n=10, ndiag=2, offs=[3, 4], ld=7, align=1),
               dict(n=10, ndiag=2, offs=[-3, 4], ld=7, align=2), dict(n=10, ndiag=1, offs=[12], ld=0, align=0)):
        rc, _, res = _refusal(eu, **kw)
        assert rc == 0 and res[0] == dc.nnz_of(kw["offs"], 10), kw
    # 2049 offsets at n = 2^20 stay below 2^31 - 1 wherever they lie (the centred band is the largest: 2 147 482 624), so the
    # overflow needs one more; the pointer outputs are NULL and nothing of that size is allocated
    centred = list(range(-1024, 1025))
    rc, _, res = _refusal(eu, big, len(centred), centred, big, 0)
    assert len(centred) == 2049 and rc == 0 and res == [2049 * big - 1024 * 1025, 2049, -1024, 1024] and res[0] <= 0x7fffffff


def test_creator_refuses_without_a_device(eu):
    """the checks of the creator that come before any device work answer on a machine without a GPU: same function, same words"""
    lib = eu._lib.load()
    offs = np.array([0, 1, 1], dtype=np.int64)
    h = ctypes.c_void_p(0x1234)
    assert lib.expv_mi_op_create_dia_loc(None, 0, 4, 3, offs.ctypes.data, None, 4, 0, 1, None) == ARGUMENT_ERROR
    assert lib.expv_mi_last_error(None).decode() == "op_create_dia: null output"
    for args, msg in (((None, 0, 4, 3, offs.ctypes.data, None, 4, 0, 1), "offset array contains duplicate values"),
                      ((None, 0, 4, 2, offs.ctypes.data, None, 3, 0, 1), "ld is smaller than a diagonal's extent"),
                      ((None, 0, 4, 2, offs.ctypes.data, None, 4, 5, 1), "unknown align"),
                      ((None, 0, 4, 2, offs.ctypes.data, None, 4, 0, 1), "null data"),
                      ((None, 0, 4, 2, offs.ctypes.data, offs.ctypes.data, 4, 0, 7), "bad location")):
        assert lib.expv_mi_op_create_dia_loc(*args, ctypes.byref(h)) == ARGUMENT_ERROR
        assert lib.expv_mi_last_error(None).decode() == "op_create_dia: " + msg
        assert h.value == 0x1234                                                          # *op untouched


# ------------------------------------------------------------------ the boundary
def test_the_new_prototypes_are_declared_exported_and_bound(eu):
    raw = open(os.path.join(ROOT, "include", "expv_mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "exponentialutilities.jl_amd", "libexpv_mi.so"))
    L = eu._lib
    for name, nargs, must in (("expv_mi_op_create_dia_loc", 10, ("int64_t n", "int ndiag", "const int64_t *offsets_host", "const void *data",
                                                                 "int64_t ld", "int align", "int loc", "expv_mi_op_t *op")),
                              ("expv_mi_host_dia_pattern", 9, ("int64_t n", "int ndiag", "const int64_t *offsets", "int64_t ld", "int align",
                                                               "int32_t *rowptr", "int32_t *colind", "int64_t *src", "int64_t out[4]"))):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
        assert m, "%s is not declared in include/expv_mi.h" % name
        args = [" ".join(a.split()) for a in abi._split_top(m.group(1))]
        assert len(args) == nargs and all(a in args for a in must), args
        assert hasattr(lib, name), "%s is not exported" % name
        res, bound = L.PROTOTYPES[name]
        assert res is ctypes.c_int and len(bound) == nargs
    enum = re.search(r"enum\s*\{([^}]*EXPV_MI_DIA_ALIGN_COL[^}]*)\}", hdr).group(1)
    vals = dict(re.findall(r"(EXPV_MI_DIA_[A-Z_]+)\s*=\s*(\d+)", enum))
    assert vals == {"EXPV_MI_DIA_ALIGN_COL": "0", "EXPV_MI_DIA_ALIGN_ROW": "1", "EXPV_MI_DIA_ALIGN_START": "2"}
    assert (L.DIA_ALIGN_COL, L.DIA_ALIGN_ROW, L.DIA_ALIGN_START) == (0, 1, 2) and dc.ALIGN_CODE == {"col": 0, "row": 1, "start": 2}
    flat = re.sub(r"\s*\n \*\s*", " ", raw)                        # (comment lines joined)
    for clause in ("THE PATTERN IS DECIDED BY THE OFFSETS ALONE", "PADDING IS NEVER READ", "offset array contains duplicate values"):
        assert clause in flat
    assert callable(eu.MIOperator.from_dia) and "host_dia_pattern" in eu.__all__


def test_julia_shim_takes_stored_diagonals():
    src = open(os.path.join(ROOT, "julia", "MIKrylov.jl")).read()
    assert ":expv_mi_op_create_dia_loc, lib" in src
    for T in ("Tridiagonal", "SymTridiagonal", "Bidiagonal", "Diagonal"):
        assert re.search(r"dia_parts\(A::%s\)" % T, src), T
    assert re.search(r"format::Symbol = :dia, align::Symbol = :col", src) and ":start => 2" in src
    abi.test_julia_shim_calls_match_the_header()
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "expv_mi_op_create_dia_loc" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_tile_constants_are_readable_and_the_source_is_built():
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_dia.hip")).read()
    c = parse_constants(src)
    assert c["DIA_TILE"] == 256 and c["DIA_TILE"] % c["DIA_TILE_MIN"] == 0 and 1 <= c["DIA_Q_FULL"] < c["DIA_Q_LDS"]
    # the staged image of every band up to DIA_Q_FULL keeps the whole tile for 16-byte elements; the widest staged band fits the
    # smallest tile; a workgroup stays inside 64 KiB of LDS
    assert ((c["DIA_Q_FULL"] | 1) * c["DIA_TILE"] * 16) <= c["DIA_LDS_BYTES"] < ((c["DIA_Q_FULL"] + 2) | 1) * c["DIA_TILE"] * 16
    assert ((c["DIA_Q_LDS"] | 1) * c["DIA_TILE_MIN"] * 16) <= c["DIA_LDS_BYTES"] and c["DIA_LDS_BYTES"] + 8 * (c["DIA_TILE"] + 1) <= 64 * 1024
    assert "op_dia.hip" in open(os.path.join(ROOT, "exponentialutilities.jl_amd", "build.py")).read()
    assert "tests/" not in src and "pytest" not in src and "asm" not in src


# ------------------------------------------------------------------ the Python helpers
def test_a_scipy_dia_matrix_with_short_rows_is_padded(eu):
    n = 9
    short = np.arange(1.0, 13.0).reshape(2, 6)                       # data.shape[1] = 6 < n: the missing slots are absent entries
    A = sp.dia_matrix((short, [0, 2]), shape=(n, n))
    data, offs, n2 = eu.api._dia_from_scipy(A)
    assert n2 == n and data.shape == (2, n) and list(offs) == [0, 2] and offs.dtype == np.int64
    assert np.array_equal(data[:, :6], short) and np.all(data[:, 6:] == 0)
    assert np.array_equal(dc.scalar_matrix(data, offs, n).toarray(), A.toarray())
    full = sp.dia_matrix((np.ones((2, n)), [0, 2]), shape=(n, n))
    assert eu.api._dia_from_scipy(full)[0] is full.data              # nothing to pad: no copy
    assert eu.api._is_scipy_dia(A) and not eu.api._is_scipy_dia(A.tocsr()) and not eu.api._is_scipy_dia(short)
    with pytest.raises(eu.DimensionMismatch, match="square"):
        eu.api._dia_from_scipy(sp.dia_matrix((short, [0, 2]), shape=(n, n + 1)))


def test_data_layout_is_taken_as_it_is_or_refused(eu):
    lay = eu.api._dia_layout
    buf = torch.arange(40, dtype=torch.float64).reshape(4, 10)
    keep, ptr, ld, loc = lay(buf[:, 1:8], np.dtype(np.float64))      # a view into a wider buffer, one element in: no copy
    assert (ld, loc) == (10, eu._lib.HOST) and ptr == buf.data_ptr() + 8 and keep.shape == (4, 7)
    assert lay(buf[:1, :7], np.dtype(np.float64))[2] == 7           # one row: its length
    assert lay(buf.numpy(), np.dtype(np.float32))[0].dtype == np.float32
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        lay(buf.t(), np.dtype(np.float64))
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        lay(buf[:, ::2], np.dtype(np.float64))
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        lay(np.asfortranarray(buf.numpy()), np.dtype(np.float64))
    with pytest.raises(ValueError, match=r"stride\(0\)"):
        lay(torch.zeros(1, 10, dtype=torch.float64).expand(4, 10), np.dtype(np.float64))
    with pytest.raises(eu.DimensionMismatch, match="2-D"):
        lay(torch.zeros(10, dtype=torch.float64), np.dtype(np.float64))
    with pytest.raises(ValueError, match="align"):
        eu.MIOperator.from_dia(buf, [0, 1, 2, 3], align="diag")
    with pytest.raises(TypeError, match="data and offsets"):
        eu.MIOperator.from_dia(buf)
