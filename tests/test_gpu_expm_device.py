"""exponential!(A) for a dense matrix on the device (expv_mi_expm) and the matrix-core product behind it (expv_mi_gemm): the dense half
of the reference's GPU tests, test/gpu/gputests.jl:22-39.

Products are checked EXACTLY: small-integer operands make every partial sum an integer far below 2^24, so each element type must give
numpy's result bit for bit, whatever order the matrix cores add in.  Exponentials are checked against scipy.linalg.expm in double
precision of the same (rounded) matrix in the Frobenius norm, at the bars the project already holds its host routine to
(tests/test_abi_cpu.py: 1e-11 for the 64-bit types, 1e-4 for the 32-bit ones; the same arithmetic on the CPU reaches 8.4e-15 / 3.6e-6
on these inputs)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import scipy.linalg as sl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARGUMENT_ERROR = 0, 2
HOST, DEVICE = 0, 1
TYPES = [np.float64, np.complex128, np.float32, np.complex64]
TOL = {np.dtype(np.float64): 1e-11, np.dtype(np.complex128): 1e-11, np.dtype(np.float32): 1e-4, np.dtype(np.complex64): 1e-4}
SIZES = [1, 2, 7, 33, 96, 129, 256]
SCALES = [None, 30.0, 1.5, 0.5, 0.1, 0.005]          # None: randn as drawn; the rest: scaled to that 1-norm (Pade 13, 9, 7, 5, 3)
PARITY_LOG = []


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module", autouse=True)
def _write_parity_log():
    yield
    if not PARITY_LOG:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "expm_device_parity.txt"), "w") as f:
            f.write("# expv_mi_expm against scipy.linalg.expm (complex128) of the same rounded matrix: relative Frobenius error\n")
            f.write("# written by tests/test_gpu_expm_device.py (-m gpu); bars: 1e-11 (float64 / complex128), 1e-4 (float32 / complex64)\n")
            f.write("# %-11s %5s %-10s %5s %3s %5s  %s\n" % ("dtype", "n", "case", "order", "s", "swaps", "rel_err"))
            for row in PARITY_LOG:
                f.write("%-13s %5d %-10s %5d %3d %5d  %.3e\n" % row)
    except OSError:
        pass


def _code(eu, T):
    return eu.api._code(np.dtype(T))


def _expected_method(nA):
    """Pade order and squarings the thresholds give (exp_baseexp.jl / host_dense.h)"""
    if nA <= 2.1:
        return (9 if nA > 0.95 else 7 if nA > 0.25 else 5 if nA > 0.015 else 3), 0
    return 13, max(0, math.ceil(math.log2(nA / 5.4)))


def _rel_err(E, ref):
    return float(np.linalg.norm(E.astype(np.complex128) - ref) / np.linalg.norm(ref))


# --------------------------------------------------------------------------------------------- the product, exact
# (m, n, k) from {1, 15, 16, 17, 31, 33, 64, 65, 129, 200}: every value in every position, non-square but for the last two
SHAPES = [(1, 15, 16), (15, 16, 17), (16, 17, 31), (17, 31, 33), (31, 33, 64), (33, 64, 65), (64, 65, 129), (65, 129, 200),
          (129, 200, 1), (200, 1, 15), (200, 129, 65), (64, 64, 64), (129, 129, 129)]
SCALARS = [(1, 0), (-1, 1), (2, -3)]


def _ints(rng, shape, T):
    a = rng.integers(-3, 4, size=shape).astype(np.float64)
    if np.dtype(T).kind == "c":
        a = a + 1j * rng.integers(-3, 4, size=shape)
    return a.astype(T)


def _padded(eu, ctx, M, extra):
    """M in a device buffer with `extra` more rows per column, the padding filled with NaN"""
    r, c = M.shape
    buf = np.full((r + extra, c), np.nan, dtype=M.dtype, order="F")
    buf[:r, :] = M
    return eu.DeviceArray.from_host(buf, ctx), r + extra


def _gemm(eu, ctx, T, m, n, k, alpha, A, lda, B, ldb, beta, Cd, ldc):
    alpha, beta = complex(alpha), complex(beta)
    return eu.api.L.load().expv_mi_gemm(ctx._h, _code(eu, T), m, n, k, alpha.real, alpha.imag, A.ptr, lda, B.ptr, ldb, beta.real, beta.imag,
                                        Cd.ptr, ldc)


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
def test_product_is_exact_on_small_integers(eu, tile_ctx, T, tile):
    ctx = tile_ctx[tile]
    rng = np.random.default_rng(42)
    scalars = SCALARS + ([(1 + 2j, -1j)] if np.dtype(T).kind == "c" else [])
    for (m, n, k) in SHAPES:
        A, B, C0 = _ints(rng, (m, k), T), _ints(rng, (k, n), T), _ints(rng, (m, n), T)
        Ad, lda = _padded(eu, ctx, A, 3)
        Bd, ldb = _padded(eu, ctx, B, 5)
        for alpha, beta in scalars:
            Cin = C0.copy()
            if beta == 0:
                Cin[...] = np.nan                      # beta == 0 must not read C
            Cd, ldc = _padded(eu, ctx, Cin, 2)
            assert _gemm(eu, ctx, T, m, n, k, alpha, Ad, lda, Bd, ldb, beta, Cd, ldc) == OK
            ctx.sync()
            got = Cd.to_host()
            want = (alpha * (A.astype(np.complex128) @ B.astype(np.complex128)) + (beta * C0.astype(np.complex128) if beta != 0 else 0))
            want = want.astype(T) if np.dtype(T).kind == "c" else want.real.astype(T)
            assert np.all(np.isfinite(got[:m, :])), (m, n, k, alpha, beta)
            assert np.array_equal(got[:m, :], want), (m, n, k, alpha, beta)
            assert np.all(np.isnan(got[m:, :])), "padding rows of C were written"
        assert np.all(np.isnan(Ad.to_host()[m:, :])) and np.all(np.isnan(Bd.to_host()[k:, :]))


@pytest.mark.parametrize("tile", ["small", "big"])
@pytest.mark.parametrize("T", TYPES)
def test_product_with_identity_returns_an_asymmetric_b_untransposed(eu, tile_ctx, T, tile):
    ctx = tile_ctx[tile]
    for (k, n) in [(33, 65), (129, 17), (64, 200)]:
        B = (np.arange(k)[:, None] * 7 + np.arange(n)[None, :] * 3 - 50).astype(np.float64)      # B[i, j] != B[j, i]
        if np.dtype(T).kind == "c":
            B = B + 1j * (np.arange(k)[:, None] - 2 * np.arange(n)[None, :])
        B = B.astype(T)
        Ad, lda = _padded(eu, ctx, np.eye(k, dtype=T), 0)
        Bd, ldb = _padded(eu, ctx, B, 1)
        Cd, ldc = _padded(eu, ctx, np.full((k, n), np.nan, dtype=T), 0)
        assert _gemm(eu, ctx, T, k, n, k, 1, Ad, lda, Bd, ldb, 0, Cd, ldc) == OK
        ctx.sync()
        assert np.array_equal(Cd.to_host(), B)
        # and B I = B from the other side
        Id, ldi = _padded(eu, ctx, np.eye(n, dtype=T), 0)
        assert _gemm(eu, ctx, T, k, n, n, 1, Bd, ldb, Id, ldi, 0, Cd, ldc) == OK
        ctx.sync()
        assert np.array_equal(Cd.to_host(), B)


def test_mul_on_torch_tensors(eu, torch):
    g = torch.Generator().manual_seed(3)
    A = torch.randint(-3, 4, (70, 40), generator=g).to(torch.float64).cuda()
    B = torch.randint(-3, 4, (40, 90), generator=g).to(torch.float64).cuda()      # row-major: copied to column-major
    Cm = torch.ones(90, 70, dtype=torch.float64, device="cuda").t()               # column-major 70 x 90
    out = eu.mul_(Cm, A, B, alpha=2, beta=-1)
    assert out is Cm
    assert torch.equal(Cm, 2 * (A @ B) - 1)
    with pytest.raises(TypeError, match="column-major"):
        eu.mul_(torch.ones(70, 90, dtype=torch.float64, device="cuda"), A, B)
    with pytest.raises(eu.DimensionMismatch):
        eu.mul_(Cm, B, A)
    ctx = eu.default_context()
    p = C.c_void_p(Cm.data_ptr())
    assert eu.api.L.load().expv_mi_gemm(ctx._h, 0, 70, 90, 40, 1.0, 0.5, p, 70, p, 40, 0.0, 0.0, p, 70) == ARGUMENT_ERROR


# --------------------------------------------------------------------------------------------- the exponential, parity
@functools.lru_cache(maxsize=None)
def _case(tname, n, scale):
    """(matrix in the element type, expm of that matrix in complex128, its 1-norm): computed once per case"""
    T = np.dtype(tname)
    rng = np.random.default_rng(1000 + n)
    A0 = rng.standard_normal((n, n))
    if T.kind == "c":
        A0 = A0 + 1j * rng.standard_normal((n, n))
    A = (A0 if scale is None else scale * A0 / np.linalg.norm(A0, 1)).astype(T)
    A = np.asfortranarray(A)
    A.setflags(write=False)
    ref = sl.expm(A.astype(np.complex128))
    return A, ref, float(np.linalg.norm(A.astype(np.complex128), 1))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("T", TYPES)
def test_exponential_matches_scipy_for_every_pade_order(eu, T, n):
    seen = set()
    for scale in SCALES:
        A, ref, nA = _case(np.dtype(T).name, n, scale)
        E, info = eu.exponential(A, return_info=True)
        assert E.dtype == np.dtype(T) and E.shape == (n, n)
        err = _rel_err(E, ref)
        order, s = _expected_method(nA)
        print("%s n=%d case=%s order=%d s=%d swaps=%d err=%.3e" % (np.dtype(T).name, n, scale, info["order"], info["squarings"],
                                                                 info["row_exchanges"], err))
        PARITY_LOG.append((np.dtype(T).name, n, "randn" if scale is None else "norm=%g" % scale, info["order"], info["squarings"],
                           info["row_exchanges"], err))
        assert (info["order"], info["squarings"]) == (order, s), (scale, nA, info)
        assert err < TOL[np.dtype(T)], (scale, err)
        if scale is not None:
            seen.add(info["order"])
    assert seen == {3, 5, 7, 9, 13}


def test_the_reference_gpu_testset(eu, torch):
    """test/gpu/gputests.jl:22-39: n = 256, Float32 randn; exponential!(copy(A_d)) and exponential!(copy(A_d), ExpMethodHigham2005(false))
    must be `≈` exp(A), i.e. within rtol = sqrt(eps(Float32)) in the Frobenius norm."""
    n = 256
    A = np.random.default_rng(0x0451).standard_normal((n, n)).astype(np.float32)
    ref = sl.expm(A.astype(np.float64))
    A_d = torch.from_numpy(A).cuda()
    E_d = eu.exponential_(A_d.clone())
    assert E_d.dtype == torch.float32 and E_d.is_cuda
    E = E_d.cpu().numpy().astype(np.float64)
    rtol = math.sqrt(np.finfo(np.float32).eps)
    err = np.linalg.norm(E - ref)
    print("gputests.jl:36  |E - exp(A)| / max(|E|, |exp(A)|) = %.3e (rtol %.3e)" % (err / max(np.linalg.norm(E), np.linalg.norm(ref)), rtol))
    assert err <= rtol * max(np.linalg.norm(E), np.linalg.norm(ref))
    assert torch.equal(A_d, torch.from_numpy(A).cuda())          # exponential!(copy(A_d)) left A_d alone


# --------------------------------------------------------------------------------------------- pivoting
def _rotation(T, n, kind):
    """kind "real": pi [[0, I], [-I, 0]]; "imag": i pi [[0, I], [I, 0]] -- both have exp(A) = -I and a leading block of V - U that is
    ~eps of its largest entry, so every correct partial pivoting exchanges n / 2 rows"""
    h = n // 2
    A = np.zeros((n, n), dtype=np.complex128)
    if kind == "real":
        A[:h, h:] = np.pi * np.eye(h)
        A[h:, :h] = -np.pi * np.eye(h)
    else:
        A[:h, h:] = 1j * np.pi * np.eye(h)
        A[h:, :h] = 1j * np.pi * np.eye(h)
    return A.astype(T) if np.dtype(T).kind == "c" else A.real.astype(T)


@pytest.mark.parametrize("n", [2, 34, 130])
@pytest.mark.parametrize("T,kind", [(T, "real") for T in TYPES] + [(np.complex128, "imag"), (np.complex64, "imag")])
def test_the_solve_pivots(eu, T, kind, n):
    A = _rotation(T, n, kind)
    ref = sl.expm(A.astype(np.complex128))
    assert np.linalg.norm(ref + np.eye(n)) < 1e-5 * math.sqrt(n)          # exp(A) = -I (A rounded to the element type)
    E, info = eu.exponential(A, return_info=True)
    err = _rel_err(E, ref)
    print("%s %s n=%d swaps=%d err=%.3e" % (np.dtype(T).name, kind, n, info["row_exchanges"], err))
    assert (info["order"], info["squarings"]) == (13, 0)
    assert info["row_exchanges"] >= n // 2
    assert err < TOL[np.dtype(T)]


# --------------------------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("T", TYPES)
def test_leading_dimension_host_device_and_layouts(eu, torch, T):
    n, lda = 45, 53
    A, ref, _ = _case(np.dtype(T).name, 96, 1.5)
    A = np.asfortranarray(A[:n, :n])
    ref = sl.expm(A.astype(np.complex128))
    lib, ctx = eu.api.L.load(), eu.default_context()
    buf = np.full((lda, n), np.nan, dtype=T, order="F")
    buf[:n, :] = A
    # loc = HOST, lda > n: sentinels survive
    h = buf.copy(order="F")
    assert lib.expv_mi_expm(ctx._h, _code(eu, T), n, h.ctypes.data, lda, HOST, None) == OK
    assert np.all(np.isnan(h[n:, :])) and _rel_err(h[:n, :], ref) < TOL[np.dtype(T)]
    # loc = DEVICE on the same bytes: the same bits, sentinels survive
    d = eu.DeviceArray.from_host(buf, ctx)
    info = (C.c_int64 * 8)()
    assert lib.expv_mi_expm(ctx._h, _code(eu, T), n, d.ptr, lda, DEVICE, info) == OK
    g = d.to_host()
    assert np.all(np.isnan(g[n:, :])) and np.array_equal(g[:n, :], h[:n, :])
    order, sq = _expected_method(float(np.linalg.norm(A.astype(np.complex128), 1)))
    assert (info[0], info[1]) == (order, sq) and info[3] > 0 and list(info[4:8]) == [0, 0, 0, 0]
    # a row-major torch tensor of an asymmetric A gives exp(A), not its transpose; a column-major one and a strided view too
    t_row = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    assert t_row.is_contiguous()
    e_row = eu.exponential_(t_row).cpu().numpy()
    assert _rel_err(e_row, ref) < TOL[np.dtype(T)] and _rel_err(e_row, ref.T) > 1e-2
    t_col = torch.from_numpy(np.ascontiguousarray(A.T)).cuda().t()
    assert t_col.stride(0) == 1
    assert np.array_equal(eu.exponential_(t_col).cpu().numpy(), h[:n, :])
    big = torch.zeros(2 * n, 2 * n, dtype=t_row.dtype, device="cuda")
    view = big[::2, ::2]
    view.copy_(torch.from_numpy(np.ascontiguousarray(A)).cuda())
    assert _rel_err(eu.exponential_(view).cpu().numpy(), ref) < TOL[np.dtype(T)]
    assert float(big[1::2, :].abs().sum()) == 0.0
    # numpy in place, DeviceArray in place
    a = np.array(A, order="F")
    assert eu.exponential_(a) is a and np.array_equal(a, h[:n, :])
    da = eu.DeviceArray.from_host(A, ctx)
    assert eu.exponential_(da) is da and np.array_equal(da.to_host(), h[:n, :])


def test_workspace_reuse_reproduces_bits(eu):
    ctx = eu.Context()
    A1, _, _ = _case("float64", 129, None)
    A2, _, _ = _case("float64", 33, 1.5)
    A3, _, _ = _case("complex64", 256, 30.0)
    first = eu.exponential(A1, ctx=ctx)
    eu.exponential(A2, ctx=ctx)
    eu.exponential(A3, ctx=ctx)
    again = eu.exponential(A1, ctx=ctx)
    assert np.array_equal(first, again)


@pytest.mark.parametrize("T", TYPES)
def test_nonfinite_input_and_empty_matrix(eu, T):
    lib, ctx = eu.api.L.load(), eu.default_context()
    A, _, _ = _case(np.dtype(T).name, 33, 1.5)
    for bad in (np.nan, np.inf):
        B = np.array(A, order="F")
        B[7, 20] = bad
        keep = B.copy()
        with pytest.raises(eu.ExpvMIError, match="matrix contains Infs or NaNs") as ei:
            eu.exponential_(B)
        assert ei.value.code == ARGUMENT_ERROR
        assert np.array_equal(B, keep, equal_nan=True)
        d = eu.DeviceArray.from_host(B, ctx)
        assert lib.expv_mi_expm(ctx._h, _code(eu, T), 33, d.ptr, 33, DEVICE, None) == ARGUMENT_ERROR
        assert np.array_equal(d.to_host(), keep, equal_nan=True)
    assert lib.expv_mi_expm(ctx._h, _code(eu, T), 0, None, 0, DEVICE, None) == OK
    E = eu.exponential(np.zeros((0, 0), dtype=T))
    assert E.shape == (0, 0)


def test_zero_matrix_gives_the_identity_without_exchanges(eu):
    E, info = eu.exponential(np.zeros((40, 40)), return_info=True)
    assert np.array_equal(E, np.eye(40)) and info["row_exchanges"] == 0 and (info["order"], info["squarings"]) == (3, 0)
