"""phi!(out, A, k) for a dense matrix on the device (expv_mi_phi; phi.jl:159-257), against the CPU sides of tests/phi_cases.py.

Parity: every phi_j against the first block row of scipy.linalg.expm of the block-augmented matrix in complex128, relative Frobenius
error at the bars the dense exponential is held to (1e-11 for the 64-bit types, 1e-4 for the 32-bit ones; the same arithmetic on the
CPU stays below 4e-15 / 2.4e-6 on these inputs, tests/test_phi_device_cpu.py).  Where the error grows with the scalings (norm 1000,
the nilpotent entry 1e6) the bar is 8 x the error of the CPU restatement on the same input -- its worst over phi_0 .. phi_k: on the
nilpotent input single phi_j of the restatement are exact, which says nothing about another order of the same roundings."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dense_cases as dc
from tests import phi_cases as pc

pytestmark = pytest.mark.gpu
OK, ARGUMENT_ERROR = 0, 2
HOST, DEVICE = 0, 1
TYPES = [np.dtype(t) for t in pc.TYPES]


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _code(eu, T):
    return eu.api._code(np.dtype(T))


def _ptrs(*p):
    return (C.c_void_p * len(p))(*[int(v) for v in p])


def _errs(phis, ref):
    return [pc.rel_err(p, r) for p, r in zip(phis, ref)]


def _check_info(T, A, k, info):
    s = pc.scalings(pc.norm1_f64(A))
    assert (info["degree"], info["scalings"], info["products"]) == (pc.degree(T), s, pc.products(T, k, s)), info


# --------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("n", pc.PARITY_SIZES)
@pytest.mark.parametrize("T", TYPES)
def test_phi_matches_the_augmented_exponential(eu, T, n):
    worst = 0.0
    for family in pc.PARITY_FAMILIES:
        for norm1 in pc.PARITY_NORMS:
            A, ref = pc.case(T.name, n, norm1, family)
            for k in pc.PARITY_ORDERS:
                phis, info = eu.phi(A, k, return_info=True)
                assert len(phis) == k + 1 and all(p.dtype == T and p.shape == (n, n) for p in phis)
                _check_info(T, A, k, info)
                errs = _errs(phis, ref)
                print("%s n=%d %s norm=%g k=%d s=%d err=%s" % (T.name, n, family, norm1, k, info["scalings"], " ".join("%.2e" % e for e in errs)))
                worst = max(worst, max(errs))
                assert max(errs) <= pc.PARITY_BAR[T.name], (family, norm1, k, errs)
    print("%s n=%d worst %.3e" % (T.name, n, worst))


# --------------------------------------------------------------------------------------------- many scalings
@pytest.mark.parametrize("family", ["skew", "negsemi"])
@pytest.mark.parametrize("T", TYPES)
def test_ten_scalings_stay_within_eight_times_the_cpu_restatement(eu, T, family):
    A = pc.matrix(T.name, 96, 1000.0, family)
    ref = pc.truth(A, 4)
    restated = max(_errs(pc.restatement(A, 4)[0], ref))
    phis, info = eu.phi(A, 4, return_info=True)
    errs = _errs(phis, ref)
    print("%s %s s=%d device %s restatement %.2e" % (T.name, family, info["scalings"], " ".join("%.2e" % e for e in errs), restated))
    assert info["scalings"] == 10
    assert max(errs) <= 8 * restated


@pytest.mark.parametrize("T", TYPES)
def test_a_nilpotent_entry_of_a_million_at_twenty_scalings(eu, T):
    A = pc.nilpotent(T, 5, 1e6)
    ref = pc.nilpotent_truth(A, 4)
    restated = max(_errs(pc.restatement(A, 4)[0], ref))
    phis, info = eu.phi(A, 4, return_info=True)
    errs = _errs(phis, ref)
    print("%s nilpotent s=%d device %s restatement %.2e" % (T.name, info["scalings"], " ".join("%.2e" % e for e in errs), restated))
    assert info["scalings"] == 20
    assert max(errs) <= 8 * restated


# --------------------------------------------------------------------------------------------- thresholds
@pytest.mark.parametrize("T", TYPES)
def test_scalings_change_exactly_at_the_thresholds(eu, T):
    R = pc.real_type(T).type
    up = lambda x: np.nextafter(R(x), R(np.inf))
    for value, s in ((R(1.0), 0), (up(1.0), 1), (R(2.0), 1), (up(2.0), 2)):
        for imaginary in ((False, True) if T.kind == "c" else (False,)):
            A = dc.threshold_matrix(T, 9, value, imaginary)
            assert pc.norm1_f64(A) == float(value)
            _, info = eu.phi(A, 2, return_info=True)
            assert (info["degree"], info["scalings"]) == (18 if R is np.float64 else 10, s), (float(value), imaginary, info)
    # the 1-norm decides, not the infinity norm: one column carries 5 over 40 rows
    A = pc.column_heavy(T, 40, 5.0)
    phis, info = eu.phi(A, 2, return_info=True)
    assert info["scalings"] == 3
    assert max(_errs(phis, pc.truth(A, 2))) <= pc.PARITY_BAR[T.name]


# --------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("T", TYPES)
def test_the_zero_matrix_gives_the_inverse_factorials_bit_for_bit(eu, T):
    n, k = 130, 4
    phis, info = eu.phi(np.zeros((n, n), dtype=T), k, return_info=True)
    assert info["scalings"] == 0
    for p, z in zip(phis, pc.zero_truth(T, n, k)):
        assert np.array_equal(p, z)


@pytest.mark.parametrize("T", TYPES)
def test_a_diagonal_matrix_gives_the_scalar_functions(eu, T):
    d = np.linspace(-6.0, 1.5, 37) * (1j if T.kind == "c" else 1)
    A = np.diag(d).astype(T)
    phis = eu.phi(A, 3)
    want = pc.diagonal_truth(np.diag(A), 3)
    assert max(_errs(phis, want)) <= pc.PARITY_BAR[T.name]
    for p in phis:
        assert np.count_nonzero(p - np.diag(np.diag(p))) == 0


@pytest.mark.parametrize("T", TYPES)
def test_transposed_storage_gives_the_transposed_functions(eu, torch, T):
    n, k = 45, 2
    A = np.asfortranarray(pc.case(T.name, 96, 5.0, "randn")[0][:n, :n])
    col = eu.phi(A, k)                                                   # numpy, column-major
    row = eu.phi(np.ascontiguousarray(A), k)                             # numpy, row-major: passed as the transposed problem
    At = eu.phi(np.asfortranarray(A.T), k)
    ref = pc.truth(A, k)
    assert max(_errs(col, ref)) <= pc.PARITY_BAR[T.name] and pc.rel_err(col[1], ref[1].T) > 1e-2
    for j in range(k + 1):
        assert row[j].strides[1] == row[j].itemsize                      # a block of a row-major slab
        assert np.array_equal(At[j].T, row[j])                           # phi_j(A') = phi_j(A)': the same device call, bit for bit
        assert pc.rel_err(row[j], ref[j]) <= pc.PARITY_BAR[T.name]
    t_row = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    got = eu.phi(t_row, k)
    assert all(g.is_cuda and g.stride(1) == 1 for g in got)
    assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, row))
    t_col = torch.from_numpy(np.ascontiguousarray(A.T)).cuda().t()
    assert t_col.stride(0) == 1
    got = eu.phi(t_col, k)
    assert all(g.stride(0) == 1 for g in got) and all(np.array_equal(g.cpu().numpy(), c) for g, c in zip(got, col))
    # A row-major, out column-major: through a copy, the same functions
    outs = [torch.empty(n, n, dtype=t_row.dtype, device="cuda").t() for _ in range(k + 1)]
    assert eu.phi_(outs, t_row, k) is outs
    assert max(_errs([o.cpu().numpy() for o in outs], ref)) <= pc.PARITY_BAR[T.name]
    assert torch.equal(t_row, torch.from_numpy(np.ascontiguousarray(A)).cuda())


# --------------------------------------------------------------------------------------------- orders
@pytest.mark.parametrize("T", TYPES)
def test_order_zero_is_the_exponential(eu, T):
    A, ref = pc.case(T.name, 65, 5.0, "randn")
    (E,), info = eu.phi(A, 0, return_info=True)
    _check_info(T, A, 0, info)
    assert pc.rel_err(E, ref[0]) <= pc.PARITY_BAR[T.name]
    P = eu.exponential(A)                                                # (Pade 13 + LU: another algorithm)
    assert pc.rel_err(E, P.astype(np.complex128)) <= pc.PARITY_BAR[T.name]


@pytest.mark.parametrize("T", TYPES)
def test_order_sixteen(eu, T):
    A = pc.matrix(T.name, 5, 5.0, "randn", seed=16)
    ref = pc.truth(A, 16)
    phis, info = eu.phi(A, 16, return_info=True)
    _check_info(T, A, 16, info)
    errs = _errs(phis, ref)
    print(T.name, "k=16", " ".join("%.1e" % e for e in errs))
    assert len(phis) == 17 and max(errs) <= pc.PARITY_BAR[T.name]


def test_orders_outside_the_limit_are_refused_and_out_is_untouched(eu):
    lib, ctx = eu.api.L.load(), eu.default_context()
    A = eu.DeviceArray.from_host(np.eye(4), ctx)
    slab = eu.DeviceArray.from_host(np.full((4, 4 * 18), 7.0), ctx)
    o = _ptrs(*[slab.ptr + j * 16 * 8 for j in range(18)])
    for k in (17, -1):
        assert lib.expv_mi_phi(ctx._h, _code(eu, np.float64), 4, k, A.ptr, 4, o, 4, DEVICE, None) == ARGUMENT_ERROR
    assert np.all(slab.to_host() == 7.0)
    assert lib.expv_mi_phi(ctx._h, _code(eu, np.float64), 4, 16, A.ptr, 4, o, 4, DEVICE, None) == OK
    assert not np.any(slab.to_host()[:, :4 * 17] == 7.0) and np.all(slab.to_host()[:, 4 * 17:] == 7.0)


# --------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("T", TYPES)
def test_leading_dimensions_separate_outputs_and_host_staging(eu, T):
    n, k, lda, ldo = 45, 2, 53, 49
    A = np.asfortranarray(pc.case(T.name, 96, 5.0, "skew")[0][:n, :n])
    ref = pc.truth(A, k)
    lib, ctx = eu.api.L.load(), eu.default_context()
    abuf = np.full((lda, n), np.nan, dtype=T, order="F")
    abuf[:n, :] = A
    obuf = np.full((ldo, (k + 1) * n), np.nan, dtype=T, order="F")          # a padded slab: block j starts at column j n
    block = lambda base, j: base + j * n * ldo * T.itemsize
    # loc = HOST
    h = obuf.copy(order="F")
    info = (C.c_int64 * 8)()
    assert lib.expv_mi_phi(ctx._h, _code(eu, T), n, k, abuf.ctypes.data, lda, _ptrs(*[block(h.ctypes.data, j) for j in range(k + 1)]), ldo,
                           HOST, info) == OK
    assert np.all(np.isnan(h[n:, :])) and np.all(np.isnan(abuf[n:, :])) and np.array_equal(abuf[:n, :], A)
    assert max(_errs([h[:n, j * n:(j + 1) * n] for j in range(k + 1)], ref)) <= pc.PARITY_BAR[T.name]
    s = pc.scalings(pc.norm1_f64(A))
    assert list(info[:3]) == [pc.degree(T), s, pc.products(T, k, s)] and info[3] > 0 and list(info[4:8]) == [0, 0, 0, 0]
    # loc = DEVICE on the same bytes: the same bits, sentinels survive, A unmodified
    ad, od = eu.DeviceArray.from_host(abuf, ctx), eu.DeviceArray.from_host(obuf, ctx)
    assert lib.expv_mi_phi(ctx._h, _code(eu, T), n, k, ad.ptr, lda, _ptrs(*[block(od.ptr, j) for j in range(k + 1)]), ldo, DEVICE, None) == OK
    g = od.to_host()
    assert np.all(np.isnan(g[n:, :])) and np.array_equal(g[:n, :], h[:n, :])
    assert np.array_equal(ad.to_host(), abuf, equal_nan=True)
    # separate matrices and one slab: identical bits (numpy, DeviceArray)
    sep = [np.empty((n, n), dtype=T, order="F") for _ in range(k + 1)]
    slab = np.empty((n, (k + 1) * n), dtype=T, order="F")
    assert eu.phi_(sep, A, k) is sep and eu.phi_(slab, A, k) is slab
    for j in range(k + 1):
        assert np.array_equal(sep[j], h[:n, j * n:(j + 1) * n]) and np.array_equal(slab[:, j * n:(j + 1) * n], sep[j])
    da = eu.DeviceArray.from_host(A, ctx)
    dsep = [eu.DeviceArray((n, n), T, ctx) for _ in range(k + 1)]
    dslab = eu.DeviceArray((n, (k + 1) * n), T, ctx)
    eu.phi_(dsep, da, k)
    eu.phi_(dslab, da, k)
    assert np.array_equal(dslab.to_host(), slab) and all(np.array_equal(d.to_host(), s_) for d, s_ in zip(dsep, sep))
    assert np.array_equal(da.to_host(), A)
    assert all(np.array_equal(v.to_host(), s_) for v, s_ in zip(eu.phi(da, k), sep))


# --------------------------------------------------------------------------------------------- both tiles of the product
@pytest.fixture(scope="module")
def tile_ctx(eu):
    """one context per tile of the product kernel (a context reads EXPV_MI_DENSE_TILE when it is created: 1 small, 2 big)"""
    out = {}
    old = os.environ.get("EXPV_MI_DENSE_TILE")
    try:
        for name, v in (("small", "1"), ("big", "2")):
            os.environ["EXPV_MI_DENSE_TILE"] = v
            out[name] = eu.Context()
    finally:
        if old is None:
            os.environ.pop("EXPV_MI_DENSE_TILE", None)
        else:
            os.environ["EXPV_MI_DENSE_TILE"] = old
    return out


@pytest.mark.parametrize("tile", ["small", "big"])
@pytest.mark.parametrize("T", TYPES)
def test_the_wide_product_on_either_tile(eu, tile_ctx, T, tile):
    A, ref = pc.case(T.name, 129, 30.0, "randn")
    phis, info = eu.phi(A, 4, ctx=tile_ctx[tile], return_info=True)
    assert info["scalings"] == 5
    assert max(_errs(phis, ref)) <= pc.PARITY_BAR[T.name]


# --------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("T", TYPES)
def test_nonfinite_input_overlap_and_empty_matrix(eu, T):
    lib, ctx = eu.api.L.load(), eu.default_context()
    n, k = 33, 2
    A = pc.case(T.name, 33, 5.0, "randn")[0]
    for bad in (np.nan, np.inf):
        B = np.array(A, order="F")
        B[7, 20] = bad
        out = np.full((n, (k + 1) * n), 7, dtype=T, order="F")
        with pytest.raises(eu.ExpvMIError, match="matrix contains Infs or NaNs") as ei:
            eu.phi_(out, B, k)
        assert ei.value.code == ARGUMENT_ERROR and np.all(out == 7)
        bd, od = eu.DeviceArray.from_host(B, ctx), eu.DeviceArray.from_host(out, ctx)
        o = _ptrs(*[od.ptr + j * n * n * T.itemsize for j in range(k + 1)])
        assert lib.expv_mi_phi(ctx._h, _code(eu, T), n, k, bd.ptr, n, o, n, DEVICE, None) == ARGUMENT_ERROR
        assert np.all(od.to_host() == 7)
    ad, od = eu.DeviceArray.from_host(A, ctx), eu.DeviceArray.from_host(np.full((n, 2 * n), 7, dtype=T), ctx)
    o = _ptrs(od.ptr, od.ptr + n * n * T.itemsize, ad.ptr + (n * n - 1) * T.itemsize)         # out[2] starts on A's last entry
    assert lib.expv_mi_phi(ctx._h, _code(eu, T), n, k, ad.ptr, n, o, n, DEVICE, None) == ARGUMENT_ERROR
    o = _ptrs(od.ptr, od.ptr + n * n * T.itemsize, od.ptr + (n * n - 1) * T.itemsize)         # out[2] starts on out[0]'s last entry
    assert lib.expv_mi_phi(ctx._h, _code(eu, T), n, k, ad.ptr, n, o, n, DEVICE, None) == ARGUMENT_ERROR
    assert np.all(od.to_host() == 7) and np.array_equal(ad.to_host(), A)
    assert lib.expv_mi_phi(ctx._h, _code(eu, T), 0, 3, None, 0, None, 0, DEVICE, None) == OK
    assert [p.shape for p in eu.phi(np.zeros((0, 0), dtype=T), 2)] == [(0, 0)] * 3


# --------------------------------------------------------------------------------------------- reuse
@pytest.mark.parametrize("async_outputs", [False, True])
def test_workspace_reuse_and_growth_reproduce_bits(eu, async_outputs):
    ctx = eu.Context(async_outputs=async_outputs)
    small, sref = pc.case("float64", 33, 5.0, "randn")
    big, bref = pc.case("complex64", 129, 30.0, "skew")

    def run(A, k):
        d = eu.DeviceArray.from_host(A, ctx)
        out = eu.phi(d, k, ctx=ctx)
        ctx.sync()
        return [o.to_host() for o in out]

    s1 = run(small, 1)
    s2 = run(small, 1)                       # back to back on one workspace
    b1 = run(big, 4)                         # larger (n, k): the workspace grows
    s3 = run(small, 1)                       # ... and serves the smaller call again
    b2 = run(big, 4)
    assert all(np.array_equal(a, b) for a, b in zip(s1, s2)) and all(np.array_equal(a, b) for a, b in zip(s1, s3))
    assert all(np.array_equal(a, b) for a, b in zip(b1, b2))
    assert max(_errs(s1, sref)) <= 1e-11 and max(_errs(b1, bref)) <= 1e-4
