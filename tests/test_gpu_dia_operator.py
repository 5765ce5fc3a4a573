"""Sparse operators created from stored diagonals (expv_mi_op_create_dia_loc, MIOperator.from_dia).

The yardstick is the operator expv_mi_op_create_csr_loc makes, on the same context, of the scalar arrays the position contract
gives (tests/dia_cases.py: expand): from the checked scalar arrays on the two take the same tail, so n, nnz, ishermitian,
opnorm_inf, the path flags, matvec and arnoldi / expv / phiv are compared for bit equality.  Every slot of `data` that corresponds
to no matrix position holds NaN throughout: an operator that read one would not be finite."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import dia_cases as dc
from tests.limits import parse_constants
from tests.test_gpu_bsr_operator import ingest, same_everything
from tests.test_gpu_device_operator import ARGUMENT_ERROR, DTYPES, RawOp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = parse_constants(open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "op_dia.hip")).read())
DIA_TILE, DIA_TILE_MIN, DIA_Q_LDS, DIA_LDS_BYTES = K["DIA_TILE"], K["DIA_TILE_MIN"], K["DIA_Q_LDS"], K["DIA_LDS_BYTES"]
OFFS = [1, -17, 17, 0, -1]                                   # (-17, -1, 0, 1, 17), scrambled
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def tile_rows(q, itemsize):
    """op_dia.hip, dia_rows: the rows a workgroup owns"""
    rows = DIA_TILE
    if q <= DIA_Q_LDS:
        while rows > DIA_TILE_MIN and (q | 1) * rows * itemsize > DIA_LDS_BYTES:
            rows //= 2
    return rows


def twin(eu, ctx, data, offsets, n, align):
    """the operator expv_mi_op_create_csr_loc makes of the restatement's scalar arrays, on the device"""
    rp, ci, va, _ = dc.expand(data, offsets, n, align)
    assert np.all(np.isfinite(va))
    arrs = [eu.DeviceArray.from_host(rp.astype(np.int32), ctx)]
    if len(ci):
        arrs += [eu.DeviceArray.from_host(ci.astype(np.int32), ctx), eu.DeviceArray.from_host(np.ascontiguousarray(va), ctx)]
    p = [a.ptr for a in arrs] + [None, None]
    h = C.c_void_p()
    eu.api._check(eu._lib.load().expv_mi_op_create_csr_loc(ctx._h, dc.DTYPE_CODE[np.dtype(data.dtype).name], n, len(ci), p[0], p[1], p[2],
                                                           4, 0, 1, C.byref(h)), ctx._h)
    return RawOp(eu, ctx, h)


def on_device(torch, data, shift=0):
    """data as a device tensor whose first element lies `shift` elements into a 256-byte aligned allocation"""
    t = torch.as_tensor(np.ascontiguousarray(data))
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device="cuda")
    view = buf[shift:].view(t.shape)
    view.copy_(t)
    return view


def case(offsets, n, T, align, ld=None, seed=7):
    diags = dc.random_diagonals(offsets, n, T, seed)
    return dc.pack(diags, offsets, n, align, T, ld=ld)


def check(eu, torch, ctx, data, offsets, n, align, T, what, shift=0, opnorm=True):
    ref = twin(eu, ctx, data, offsets, n, align)
    op = eu.MIOperator.from_dia(on_device(torch, data, shift), offsets, n, align, ctx=ctx)
    assert op.shape == (n, n) and op.nnz == dc.nnz_of(offsets, n), what
    same_everything(eu, ctx, op, ref, T, what, opnorm=opnorm)
    return op, ref


# ------------------------------------------------------------------ 1. same operator, same bits
COMBOS = [(np.float64, "col", "tensor"), (np.complex128, "row", "tensor"), (np.float32, "start", "tensor"), (np.complex64, "col", "scipy"),
          (np.float64, "start", "numpy"), (np.complex128, "col", "scipy"), (np.float32, "row", "numpy"), (np.complex64, "start", "tensor")]
assert {c[0] for c in COMBOS} == set(DTYPES) and {c[1] for c in COMBOS} == set(dc.ALIGNS)


@pytest.mark.parametrize("T,align,how", COMBOS)
def test_scrambled_pentadiagonal_gives_the_csr_born_operator_bit_for_bit(eu, torch, T, align, how):
    n = 300
    data = case(OFFS, n, T, align, ld=n if how == "scipy" else None)
    what = "%s %s %s" % (np.dtype(T).name, align, how)
    ctx = eu.Context()
    ref = twin(eu, ctx, data, OFFS, n, align)
    if how == "tensor":
        op = eu.MIOperator.from_dia(on_device(torch, data), torch.as_tensor(OFFS), n, align, ctx=ctx)
    elif how == "numpy":
        op = eu.MIOperator.from_dia(data, OFFS, n, align, ctx=ctx)
    else:
        op = eu.MIOperator.from_dia(sp.dia_matrix((data, OFFS), shape=(n, n)), ctx=ctx)
    assert op.shape == (n, n) and op.nnz == 5 * n - 36 and op.dtype == np.dtype(T)
    same_everything(eu, ctx, op, ref, T, what)
    info = op.ingest_info
    assert info["from_device"] and info["pattern_bytes_to_host"] == 4 * (n + 1 + op.nnz) and info["value_bytes_to_host"] == 0, info
    assert info["coo_entries"] == 0 and info["sort_passes"] == 0 and ingest(op) == ingest(ref)
    # the host-born operator of the same matrix (its norm is summed on the host, in another order)
    same_everything(eu, ctx, op, eu.MIOperator(dc.scalar_matrix(data, OFFS, n, align), ctx), T, what + " vs host-born", opnorm=False)


# ------------------------------------------------------------------ 2. rows around the tile
@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("ndiag", [3, 9])
@pytest.mark.parametrize("n", [DIA_TILE - 1, DIA_TILE, DIA_TILE + 1, 2 * DIA_TILE + 3])
def test_rows_around_the_tile(eu, torch, n, ndiag, T):
    offs = dc.scramble([-1, 0, 1] if ndiag == 3 else [-40, -5, -2, -1, 0, 1, 3, 7, 64])
    assert tile_rows(ndiag, np.dtype(T).itemsize) == DIA_TILE
    ctx = eu.Context()
    for align in ("col", "start"):
        check(eu, torch, ctx, case(offs, n, T, align), offs, n, align, T, "n %d, %d diagonals, %s" % (n, ndiag, align))


# ------------------------------------------------------------------ 3. corner shapes
@pytest.mark.parametrize("T", [np.float64, np.complex128, np.float32])
def test_every_diagonal_of_a_small_matrix_takes_the_gather_form(eu, torch, T):
    n = 33
    offs = dc.scramble(list(range(-(n - 1), n)), seed=3)
    assert len(offs) == 65 > DIA_Q_LDS                         # beyond the staged form
    ctx = eu.Context()
    for align in dc.ALIGNS:
        op, _ = check(eu, torch, ctx, case(offs, n, T, align), offs, n, align, T, "dense 33 %s" % align)
        assert op.nnz == n * n


@pytest.mark.parametrize("T", [np.float64, np.complex128])
def test_band_widths_at_which_the_tile_shrinks_and_the_staged_form_ends(eu, torch, T):
    isz = np.dtype(T).itemsize
    full = max(q for q in range(1, DIA_Q_LDS + 1) if tile_rows(q, isz) == DIA_TILE)
    ctx = eu.Context()
    seen = set()
    for q in (full, full + 1, 2 * full + 2, DIA_Q_LDS, DIA_Q_LDS + 1):
        rows = tile_rows(q, isz)
        seen.add((rows, q > DIA_Q_LDS))
        n = max(2 * rows + 3, q // 2 + 2)                      # more than two tiles; every offset in range
        offs = dc.scramble(list(range(-(q // 2), q - q // 2)), seed=q)
        assert len(offs) == q and all(abs(k) < n for k in offs)
        for align in ("col", "row"):
            check(eu, torch, ctx, case(offs, n, T, align, ld=n + 1), offs, n, align, T, "q %d rows %d %s" % (q, rows, align))
    assert len({r for r, _ in seen}) >= 3 and (DIA_TILE, True) in seen and (isz < 16 or (DIA_TILE_MIN, False) in seen)


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_single_corner_entries_n_one_and_the_zero_operator(eu, torch, T):
    ctx = eu.Context()
    n = 40
    for k in (n - 1, -(n - 1)):
        for align in dc.ALIGNS:
            op, _ = check(eu, torch, ctx, case([k], n, T, align), [k], n, align, T, "one diagonal %d %s" % (k, align))
            assert op.nnz == 1
    # the corner entry among out-of-range offsets, whose whole rows are NaN
    offs = [n, n - 1, -n - 5, 3 * n]
    check(eu, torch, ctx, case(offs, n, T, "col"), offs, n, "col", T, "out of range mixed in")
    op = eu.MIOperator.from_dia(on_device(torch, np.array([[np.nan], [2.5], [np.nan]], dtype=T)), [1, 0, -1], 1, "start", ctx=ctx)
    assert op.shape == (1, 1) and op.nnz == 1 and np.array_equal(np.array(op.matvec(np.ones(1, dtype=T))), np.array([2.5], dtype=T))
    for offs in ([], [7, -7, 100]):
        m = 7
        data = np.full((len(offs), m), np.nan, dtype=T)
        for z in (eu.MIOperator.from_dia(on_device(torch, data), offs, m, ctx=ctx), eu.MIOperator.from_dia(data, offs, m, ctx=ctx)):
            assert z.shape == (m, m) and z.nnz == 0 and z.opnorm_inf == 0.0
            x = np.arange(1, m + 1).astype(T)
            assert np.array_equal(np.array(z.matvec(x)), np.zeros(m, dtype=T))
            z.update_values(data)                                # nothing to refresh, nothing read


# ------------------------------------------------------------------ 4. unfriendly buffers
@pytest.mark.parametrize("T", [np.float64, np.float32, np.complex128])
@pytest.mark.parametrize("align", dc.ALIGNS)
def test_wide_rows_and_pointers_with_and_without_alignment(eu, torch, T, align):
    n = 2 * DIA_TILE + 3
    ctx = eu.Context()
    for ld, shift in ((n + 5, 0), (n + 5, 1), (n + 8, 0), (None, 1)):      # odd row stride; one element in; rows on 16 bytes; tight
        data = case(OFFS, n, T, align, ld=ld)
        op, _ = check(eu, torch, ctx, data, OFFS, n, align, T, "ld %s shift %d %s" % (ld, shift, align), shift=shift)
    # a view into a wider tensor: stride(0) is the ld, nothing is copied
    wide = on_device(torch, np.concatenate([data, np.full((len(OFFS), 7), np.nan, dtype=T)], axis=1))
    view = wide[:, :data.shape[1]]
    assert view.stride(0) == data.shape[1] + 7 and not view.is_contiguous()
    op2 = eu.MIOperator.from_dia(view, OFFS, n, align, ctx=ctx)
    same_everything(eu, ctx, op2, op, T, "strided view %s" % align)
    with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
        eu.MIOperator.from_dia(wide.t()[:data.shape[1]].t()[:, ::2], OFFS, n, align, ctx=ctx)


# ------------------------------------------------------------------ 5. Hermitian
def test_hermitian_matrices_are_found_on_the_device(eu, torch):
    n = 300
    ctx = eu.Context()
    rng = np.random.default_rng(5)
    e = rng.standard_normal(n - 1)
    sym = {-1: e, 0: rng.standard_normal(n), 1: e.copy()}
    c1, c2 = dc.random_values(n - 1, np.complex128, rng), dc.random_values(n - 2, np.complex128, rng)
    her = {-2: np.conj(c2), -1: np.conj(c1), 0: rng.standard_normal(n).astype(np.complex128), 1: c1, 2: c2}
    for diags, T in ((sym, np.float64), (her, np.complex128)):
        offs = dc.scramble(sorted(diags))
        for align in dc.ALIGNS:
            data = dc.pack(diags, offs, n, align, T)
            op, ref = check(eu, torch, ctx, data, offs, n, align, T, "hermitian %s %s" % (np.dtype(T).name, align))
            assert op.ishermitian and ref.ishermitian and op.ingest_info["value_bytes_to_host"] == 0
        broken = {k: v.copy() for k, v in diags.items()}
        broken[1][n // 2] += 0.5
        op, ref = check(eu, torch, ctx, dc.pack(broken, offs, n, "col", T), offs, n, "col", T, "one entry off")
        assert not op.ishermitian and not ref.ishermitian and op.ingest_info["value_bytes_to_host"] == 0


# ------------------------------------------------------------------ 6. it reaches the fast path
def test_pentadiagonal_takes_the_single_pass_pipeline_in_its_diagonal_form(eu, torch):
    n, T, offs = 8192, np.float64, [2, -1, 0, -2, 1]
    data = case(offs, n, T, "col")
    assert eu.host_pattern_info(dc.scalar_matrix(data, offs, n), T)["pipeline_dia_diagonals"] == 5
    ctx = eu.Context()
    op, ref = check(eu, torch, ctx, data, offs, n, "col", T, "pentadiagonal 8192")      # path flags, reorder_info, patch_info, bits
    b = np.random.default_rng(8).standard_normal(n)
    eu.expv(0.3, ref, b, m=20)
    path = tuple(eu.expv.last_stats["path"])
    eu.expv(0.3, op, b, m=20)
    assert "pipeline" in path and tuple(eu.expv.last_stats["path"]) == path, path
    assert not op.reorder_info["reordered"] and not op.patch_info["patch_form"]
    # constant diagonals under option stencil: the diagonals go to the step as scalars
    cs = eu.Context()
    cs.set_option("stencil", 1)
    const = {-2: -1.0 / 12, -1: 4.0 / 3, 0: -2.5, 1: 4.0 / 3, 2: -1.0 / 12}
    cdata = dc.pack({k: np.full(n - abs(k), v) for k, v in const.items()}, offs, n, "row", T)
    ops, refs = check(eu, torch, cs, cdata, offs, n, "row", T, "constant diagonals, stencil = 1")
    assert ops.ishermitian and refs.ishermitian
    w1, w2 = np.array(eu.expv(0.3, ops, b, m=20)), np.array(eu.expv(0.3, refs, b, m=20))
    assert np.array_equal(w1, w2) and np.all(np.isfinite(w1)) and "pipeline" in tuple(eu.expv.last_stats["path"])


# ------------------------------------------------------------------ 7. update_values
@pytest.mark.parametrize("T", [np.float64, np.complex64])
@pytest.mark.parametrize("align", dc.ALIGNS)
def test_update_values_is_creating_anew(eu, torch, align, T):
    n = 2 * DIA_TILE + 3
    d1, d2, d3 = (case(OFFS, n, T, align, ld=n + 5, seed=s) for s in (11, 12, 13))
    ctx = eu.Context()
    op = eu.MIOperator.from_dia(on_device(torch, d1), OFFS, n, align, ctx=ctx)
    fresh = eu.MIOperator.from_dia(on_device(torch, d2), OFFS, n, align, ctx=ctx)
    assert op.update_values(on_device(torch, d2)) is op
    same_everything(eu, ctx, op, fresh, T, "update_values(device) %s" % align)
    same_everything(eu, ctx, op, twin(eu, ctx, d2, OFFS, n, align), T, "update_values(device) vs twin %s" % align)
    op.update_values(d3)                                         # host data: staged, the same kernels
    same_everything(eu, ctx, op, twin(eu, ctx, d3, OFFS, n, align), T, "update_values(host) %s" % align)
    op.update_values(on_device(torch, d1, shift=1))              # another alignment of the pointer
    same_everything(eu, ctx, op, twin(eu, ctx, d1, OFFS, n, align), T, "update_values(shifted) %s" % align)
    with pytest.raises(eu.DimensionMismatch):
        op.update_values(d3[:, :-1])
    if align == "col":
        host = eu.MIOperator.from_dia(sp.dia_matrix((d1[:, :n], OFFS), shape=(n, n)), ctx=ctx)
        host.update_values(sp.dia_matrix((d2[:, :n], OFFS), shape=(n, n)))
        same_everything(eu, ctx, host, fresh, T, "update_values(dia_matrix)")
        with pytest.raises(ValueError, match="offsets of the creation"):
            host.update_values(sp.dia_matrix((d2[:, :n], sorted(OFFS)), shape=(n, n)))
        opc = op.astype(np.complex128)
        assert opc.dtype == np.complex128 and opc.ingest_info["from_device"]
        same_everything(eu, ctx, opc, twin(eu, ctx, d1.astype(np.complex128), OFFS, n, align), np.complex128, "astype")


# ------------------------------------------------------------------ 8. loc = HOST through the C ABI, 9. refusals
def raw_create(eu, ctx, T, n, offsets, data_ptr, ld, align, loc, h=None):
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    h = C.c_void_p() if h is None else h
    rc = eu._lib.load().expv_mi_op_create_dia_loc(ctx._h, dc.DTYPE_CODE[np.dtype(T).name], n, len(offs), offs.ctypes.data if len(offs) else None,
                                                  data_ptr, ld, dc.ALIGN_CODE[align], loc, C.byref(h))
    return rc, h


@pytest.mark.parametrize("T", DTYPES)
def test_host_data_is_staged_and_takes_the_same_path(eu, torch, T):
    n = DIA_TILE + 1
    ctx = eu.Context()
    for align in dc.ALIGNS:
        data = case(OFFS + [n + 3], n, T, align, ld=n + 5)
        offs = OFFS + [n + 3]
        rc, h = raw_create(eu, ctx, T, n, offs, data.ctypes.data, n + 5, align, HOST)
        eu.api._check(rc, ctx._h)
        oph = RawOp(eu, ctx, h)
        t = on_device(torch, data)
        rc, h = raw_create(eu, ctx, T, n, offs, t.data_ptr(), n + 5, align, DEVICE)
        eu.api._check(rc, ctx._h)
        opd = RawOp(eu, ctx, h)
        same_everything(eu, ctx, oph, opd, T, "loc = HOST %s" % align)
        same_everything(eu, ctx, oph, twin(eu, ctx, data, offs, n, align), T, "loc = HOST vs twin %s" % align)
        out = (C.c_int64 * 8)()
        assert eu._lib.load().expv_mi_op_ingest_info(oph._h, out) == 0
        assert (out[0], out[1], out[2], out[6], out[7]) == (1, 4 * (n + 1 + oph.nnz), 0, 0, 0)


def test_bad_arguments_are_refused_before_any_device_work(eu, torch):
    """only checks that fire before any device work: no pointer handed over here could reach a kernel"""
    ctx = eu.Context()
    n = 50
    t = on_device(torch, case([0, 1], n, np.float64, "col"))
    lib = eu._lib.load()
    for args, msg in ((dict(offsets=[1, 0, 1], data_ptr=t.data_ptr(), ld=n, align="col", loc=DEVICE), "offset array contains duplicate values"),
                      (dict(offsets=[0, 1], data_ptr=t.data_ptr(), ld=n - 1, align="col", loc=DEVICE), "ld is smaller than a diagonal's extent"),
                      (dict(offsets=[0, 1], data_ptr=None, ld=n, align="col", loc=DEVICE), "null data"),
                      (dict(offsets=[0, 1], data_ptr=t.data_ptr(), ld=n, align="row", loc=5), "bad location")):
        h = C.c_void_p(0x1234)
        rc, h = raw_create(eu, ctx, np.float64, n, h=h, **args)
        assert rc == ARGUMENT_ERROR and lib.expv_mi_last_error(ctx._h).decode() == "op_create_dia: " + msg and h.value == 0x1234
    h = C.c_void_p(0x1234)
    offs = np.array([0, 1], dtype=np.int64)
    assert lib.expv_mi_op_create_dia_loc(ctx._h, 0, n, 2, offs.ctypes.data, t.data_ptr(), n, 3, DEVICE, C.byref(h)) == ARGUMENT_ERROR
    assert lib.expv_mi_last_error(ctx._h).decode() == "op_create_dia: unknown align" and h.value == 0x1234
    with pytest.raises(eu._lib.ExpvMIError, match="duplicate"):
        eu.MIOperator.from_dia(t, [1, 1], n, ctx=ctx)
