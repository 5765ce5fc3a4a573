"""expv_mi_expm and expv_mi_gemm past what tests/test_gpu_expm_device.py reaches (inputs and CPU sides: tests/dense_cases.py, whose
properties tests/test_expm_device_cpu.py checks without a device).

* sizes at which every loop of csrc/dense_dev.hip takes a second trip: panels taller than the panel kernel's 512 threads with pivots
  more than 512 rows down, column sums and exchanges past 256 rows / columns, the element-wise kernels past their 4096 workgroups;
* an LU that exchanges rows WITH fill: scattered skew blocks, the exchange count equal to LAPACK's on the CPU-formed V - U;
* pivot columns whose largest value occurs twice, bit for bit: the first of the two rows has to win, as in LAPACK;
* more than 8 squarings, against the same arithmetic on the CPU (the error grows like |A| eps there too, so the bar is 8 x that);
* the method thresholds at and one ulp past each of them, and a float32 column whose sum passes 0.25 only in double precision;
* two stream-ordered calls back to back on one workspace;
* the product kernel on operands spanning 2^16 in magnitude against a wider accumulation, inside the componentwise bound that holds
  for every summation order; k = 0, empty C, and the size-selected tile on both sides of its switch.

Every exponential case appends a line to profiles/expm_device_parity.txt, below the lines of tests/test_gpu_expm_device.py."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.linalg as sl

from tests import dense_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
HOST, DEVICE = 0, 1
TYPES = ["float64", "complex128", "float32", "complex64"]
TOL = {"float64": 1e-11, "complex128": 1e-11, "float32": 1e-4, "complex64": 1e-4}
MARK = "# ---- tests/test_gpu_expm_device_stress.py"
PARITY_LOG, PRODUCT_LOG = [], {}


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module", autouse=True)
def _append_parity_log():
    yield
    if not PARITY_LOG and not PRODUCT_LOG:
        return
    path = os.path.join(ROOT, "profiles", "expm_device_parity.txt")
    try:
        head = open(path).read() if os.path.exists(path) else ""
        head = head.split(MARK)[0]                # a second run replaces its own section, never the lines above it
        with open(path, "w") as f:
            f.write(head)
            f.write(MARK + " (-m gpu): scattered skew blocks against the blockwise scipy reference, thresholds, the product's error bound\n")
            f.write("# lapack: exchanges of LAPACK's getrf on the CPU-formed V - U; restated: the same algorithm in the element type on the CPU\n")
            f.write("# |a|=t, t+ulp, t-ulp: one entry of that magnitude (t rounded to the element type) carries the 1-norm, i: purely imaginary\n")
            f.write("# %-11s %5s %-16s %5s %3s %6s %6s  %-10s %-10s %s\n" % ("dtype", "n", "case", "order", "s", "swaps", "lapack", "rel_err",
                                                                             "restated", "bar"))
            for row in PARITY_LOG:
                f.write("%-13s %5d %-16s %5d %3d %6d %6s  %.3e  %-10s %.3e\n" % row)
            for tname in TYPES:
                if tname in PRODUCT_LOG:
                    f.write("# product %-10s worst |C^ - C| / (gamma (|alpha| |A| |B| + |beta| |C0|)) = %.3e  (%s)\n" % ((tname,) + PRODUCT_LOG[tname]))
    except OSError:
        pass


def _log(tname, n, case, info, lapack, err, restated, bar):
    PARITY_LOG.append((tname, n, case, info["order"], info["squarings"], info["row_exchanges"], "-" if lapack is None else "%d" % lapack, err,
                       "-" if restated is None else "%.3e" % restated, bar))
    print("%s n=%d %s order=%d s=%d swaps=%d lapack=%s err=%.3e restated=%s bar=%.3e" % PARITY_LOG[-1])


def _code(eu, T):
    return eu.api._code(np.dtype(T))


# --------------------------------------------------------------------------------------------- pivoting with fill
@pytest.mark.parametrize("n,k", [(130, 6), (545, 6), (1090, 7)])
@pytest.mark.parametrize("tname", TYPES)
def test_pivoting_with_fill_exchanges_the_rows_lapack_exchanges(eu, tname, n, k):
    """n = 1090 is the smallest of these with a panel taller than the panel kernel's 512 threads AND pivots more than 512 rows down"""
    c = dc.skew_case(tname, n, k, 5.0)
    st = c["stats"]
    # conditions on the input: it pivots with fill, and every pivot beats its runner-up by far more than the rounding of V - U
    assert st["exchanges"] >= n / 25 and st["rows_twice"] >= 5 and (n < 1090 or st["far"] >= 5)
    assert c["gap"] > 1000 * float(np.finfo(np.dtype(tname)).eps)
    E, info = eu.exponential(c["A"], return_info=True)
    err = dc.rel_err(E, c["ref"])
    _log(tname, n, "skew norm=5", info, st["exchanges"], err, c["restated_err"], TOL[tname])
    assert E.dtype == np.dtype(tname)
    assert (info["order"], info["squarings"]) == (13, 0)
    assert err < TOL[tname]
    assert info["row_exchanges"] == st["exchanges"]


@pytest.mark.parametrize("n", [130, 1090])
@pytest.mark.parametrize("tname", TYPES)
def test_the_first_of_two_exactly_tied_pivot_candidates_wins(eu, tname, n):
    """tests/dense_cases.tied_hubs: every 3 x 3 block's first pivot column holds its largest value in two rows, bit for bit on any
    product kernel whose sums over k do not depend on the row.  LAPACK's rule -- the first -- exchanges twice per block, the last
    once; at n = 1090 the two rows often sit in different trips of a panel thread's row loop, and in different waves."""
    c = dc.tied_case(tname, n)
    nb = len(c["blocks"])
    assert c["first"][0] == 2 * nb and c["last"][0] == nb and min(c["first"][2], c["last"][2]) > 0.1      # (conditions on the input)
    E, info = eu.exponential(c["A"], return_info=True)
    err = dc.rel_err(E, c["ref"])
    _log(tname, n, "tied hubs", info, 2 * nb, err, c["restated_err"], TOL[tname])
    assert (info["order"], info["squarings"]) == (13, 0)
    assert err < TOL[tname]
    assert info["row_exchanges"] == 2 * nb


# --------------------------------------------------------------------------------------------- past one pass of every loop
@pytest.mark.parametrize("tname,n,k", [("float64", 1500, 7), ("complex128", 1100, 7), ("float32", 2100, 7), ("complex64", 1500, 7)])
def test_sizes_past_the_workgroup_cap_of_the_elementwise_kernels(eu, tname, n, k):
    """the Horner update and (V + U, V - U) launch at most 4096 workgroups of 256 threads on 16-byte packs: a second grid-stride trip
    from n = 1025 (complex128), 1449 (float64, complex64), 2049 (float32)"""
    T = np.dtype(tname)
    packs = n * n * (2 if T.kind == "c" else 1) // (16 // dc.real_type(T).itemsize)
    assert packs > 4096 * 256                        # (the sizes are past the cap)
    c = dc.skew_case(tname, n, k, 5.0, False)
    E, info = eu.exponential(c["A"], return_info=True)
    err = dc.rel_err(E, c["ref"])
    _log(tname, n, "skew norm=5", info, c["stats"]["exchanges"], err, c["restated_err"], TOL[tname])
    assert (info["order"], info["squarings"]) == (13, 0)
    assert err < TOL[tname]
    assert c["stats"]["far"] >= 5
    assert 2 * info["row_exchanges"] >= c["stats"]["exchanges"]


# --------------------------------------------------------------------------------------------- more than 8 squarings
@pytest.mark.parametrize("norm1,s", [(5000.0, 10), (30000.0, 13)])
@pytest.mark.parametrize("tname", TYPES)
def test_large_norms_square_more_than_eight_times(eu, tname, norm1, s):
    """The reference's generated graph stops at 2^-8; this library does not.  Stopping there leaves Pade 13 at a norm of 19.5 (117 for 30000)
    and is wrong by orders of magnitude.  The error grows like |A| eps through the squarings in any arithmetic, so the bar is the
    same algorithm in the element type on the CPU, times 8 for the other summation order of the matrix cores and the blocked LU."""
    c = dc.skew_case(tname, 545, 6, norm1, False)
    assert (c["order"], c["s"]) == (13, s) == dc.expected_method(c["norm1"])
    E, info = eu.exponential(c["A"], return_info=True)
    err = dc.rel_err(E, c["ref"])
    bar = 8 * c["restated_err"]
    _log(tname, 545, "skew norm=%g" % norm1, info, c["stats"]["exchanges"], err, c["restated_err"], bar)
    assert (info["order"], info["squarings"]) == (13, s)
    assert np.all(np.isfinite(E))
    assert err <= bar


# --------------------------------------------------------------------------------------------- thresholds
def _up(v):
    return np.nextafter(v, type(v)(np.inf))


@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("tname", TYPES)
def test_method_selection_at_and_one_ulp_past_every_threshold(eu, tname, n):
    T = np.dtype(tname)
    R = dc.real_type(T).type
    wide = R is np.float64
    lower = {0.015: (3, 0), 0.25: (5, 0), 0.95: (7, 0), 2.1: (9, 0), 5.4: (13, 0), 10.8: (13, 1)}
    upper = {0.015: (5, 0), 0.25: (7, 0), 0.95: (9, 0), 2.1: (13, 0), 5.4: (13, 1), 10.8: (13, 2)}
    seen = set()
    for thr in lower:
        v0 = R(thr)
        for v in ((v0, _up(v0)) if wide else (np.nextafter(v0, R(0)), v0, _up(v0))):
            for imaginary in ((False, True) if T.kind == "c" else (False,)):
                A = dc.threshold_matrix(T, n, v, imaginary)
                nA = dc.norm1_f64(A)
                assert nA == float(v)
                want = dc.expected_method(nA)
                if wide:                             # stated, not computed: the lower method AT the threshold, the higher one ulp above
                    assert want == (lower[thr] if v == v0 else upper[thr]) and (float(v) == thr) == (v == v0)
                else:                                # the float32 neighbours of the threshold lie on both sides of it
                    assert want == (lower[thr] if float(v) <= thr else upper[thr])
                E, info = eu.exponential(A, return_info=True)
                err = dc.rel_err(E, sl.expm(A.astype(np.complex128)))
                case = "%s%g%s" % ("i " if imaginary else "", thr, "" if v == v0 else "+ulp" if v > v0 else "-ulp")
                _log(tname, n, "|a|=" + case, info, None, err, None, TOL[tname])
                assert (info["order"], info["squarings"]) == want, (thr, float(v), imaginary)
                assert err < TOL[tname], (thr, float(v), imaginary)
                seen.add(want)
    assert seen == set(lower.values()) | set(upper.values())


@pytest.mark.parametrize("seed", [2, 3, 5])
def test_the_norm_is_summed_in_double_precision(eu, seed):
    """a float32 column that sums to more than 0.25 in double precision and to 0.25 or less in float32, in every order tried"""
    A, j = dc.fp64_norm_matrix(300, seed)
    s64 = float(np.sum(A[:, j].astype(np.float64)))
    assert 0.25 < s64 <= 0.25 + 2e-10 and s64 == dc.norm1_f64(A)
    f32 = dc.f32_sums(A[:, j])
    assert all(v <= 0.25 for v in f32.values()), f32
    E, info = eu.exponential(A, return_info=True)
    err = dc.rel_err(E, sl.expm(A.astype(np.float64)))
    _log("float32", 300, "colsum=.25+%.0e" % (s64 - 0.25), info, None, err, None, TOL["float32"])
    assert (info["order"], info["squarings"]) == (7, 0)
    assert err < TOL["float32"]


# --------------------------------------------------------------------------------------------- stream-ordered outputs
def test_back_to_back_stream_ordered_calls_share_the_workspace(eu):
    """async_outputs: a DEVICE call returns with its last copy still in flight; the next call's status reset and workspace writes must
    stay behind it.  Both results: bit for bit those of a context that completes every call."""
    lib = eu.api.L.load()
    A1 = dc.skew_case("float64", 130, 6, 5.0)["A"]
    A2 = np.asfortranarray(np.random.default_rng(1096).standard_normal((96, 96)))
    sync_ctx = eu.Context()
    want1 = eu.exponential_(eu.DeviceArray.from_host(A1, sync_ctx)).to_host()
    want2 = eu.exponential_(eu.DeviceArray.from_host(A2, sync_ctx)).to_host()
    ctx = eu.Context(async_outputs=True)
    d1, d2 = eu.DeviceArray.from_host(A1, ctx), eu.DeviceArray.from_host(A2, ctx)
    i1, i2 = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    assert lib.expv_mi_expm(ctx._h, _code(eu, np.float64), 130, d1.ptr, 130, DEVICE, i1) == OK
    assert lib.expv_mi_expm(ctx._h, _code(eu, np.float64), 96, d2.ptr, 96, DEVICE, i2) == OK
    ctx.sync()
    got1, got2 = d1.to_host(), d2.to_host()
    assert (i1[0], i1[1]) == (13, 0) and i1[2] == dc.skew_case("float64", 130, 6, 5.0)["stats"]["exchanges"] and i2[2] == 0
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2)
    assert dc.rel_err(got2, sl.expm(A2.astype(np.complex128))) < TOL["float64"]


# --------------------------------------------------------------------------------------------- the product: precision
@pytest.fixture(scope="module")
def tile_ctx(eu):
    """one context per forced tile of the product kernel, and a default one (created with EXPV_MI_DENSE_TILE unset: tile by size)"""
    out = {}
    old = os.environ.pop("EXPV_MI_DENSE_TILE", None)
    try:
        out["by_size"] = eu.Context()
        for name, v in (("small", "1"), ("big", "2")):
            os.environ["EXPV_MI_DENSE_TILE"] = v
            out[name] = eu.Context()
    finally:
        os.environ.pop("EXPV_MI_DENSE_TILE", None)
        if old is not None:
            os.environ["EXPV_MI_DENSE_TILE"] = old
    return out


def _gemm(eu, ctx, T, m, n, k, alpha, A, lda, B, ldb, beta, Cd, ldc):
    alpha, beta = complex(alpha), complex(beta)
    ptr = lambda x: None if x is None else x.ptr
    return eu.api.L.load().expv_mi_gemm(ctx._h, _code(eu, T), m, n, k, alpha.real, alpha.imag, ptr(A), lda, ptr(B), ldb, beta.real, beta.imag,
                                        ptr(Cd), ldc)


def _wide_range(rng, shape, T):
    """randn x 2^e, e uniform in [-8, 8] per entry: magnitudes spanning 2^16"""
    def draw():
        return rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, size=shape))
    a = draw() + 1j * draw() if np.dtype(T).kind == "c" else draw()
    return np.asfortranarray(a.astype(T))


@pytest.mark.parametrize("tile", ["small", "big"])
@pytest.mark.parametrize("tname", TYPES)
def test_product_error_is_inside_the_bound_of_every_summation_order(eu, tile_ctx, tname, tile):
    """|C^ - C| <= gamma (|alpha| |A| |B| + |beta| |C0|) componentwise: a product or an accumulator carried in less than the element
    type is outside by orders of magnitude, whatever the order of the sums (alpha = -1, beta = 1 is how the LU calls the kernel)"""
    ctx, T = tile_ctx[tile], np.dtype(tname)
    rng = np.random.default_rng(77)
    worst = 0.0
    for (m, n, k) in [(65, 33, 129), (129, 200, 1000)]:
        A, B, C0 = _wide_range(rng, (m, k), T), _wide_range(rng, (k, n), T), _wide_range(rng, (m, n), T)
        Ad, Bd = eu.DeviceArray.from_host(A, ctx), eu.DeviceArray.from_host(B, ctx)
        for alpha, beta in [(1, 0), (-1, 1)]:
            Cd = eu.DeviceArray.from_host(C0 if beta else np.full((m, n), np.nan, dtype=T, order="F"), ctx)
            assert _gemm(eu, ctx, T, m, n, k, alpha, Ad, m, Bd, k, beta, Cd, m) == OK
            ctx.sync()
            got = Cd.to_host()
            assert np.all(np.isfinite(got))
            want, mag = dc.wide_product(alpha, A, B, beta, C0)
            bound = dc.product_gamma(T, k) * mag
            assert np.all(bound > 0)
            ratio = float(np.max(np.abs(got.astype(want.dtype) - want).astype(np.float64) / bound))
            print("%s %s tile (%d, %d, %d) alpha=%g beta=%g worst error / bound = %.3e" % (tname, tile, m, n, k, alpha, beta, ratio))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (m, n, k, alpha, beta)
    if worst > PRODUCT_LOG.get(tname, (0.0, ""))[0]:
        PRODUCT_LOG[tname] = (worst, tile + " tile")


# --------------------------------------------------------------------------------------------- the product: degenerate shapes, tile by size
@pytest.mark.parametrize("tile", ["small", "big", "by_size"])
@pytest.mark.parametrize("tname", TYPES)
def test_product_with_k_zero_or_an_empty_c(eu, tile_ctx, tname, tile):
    ctx, T = tile_ctx[tile], np.dtype(tname)
    m, n = 70, 37
    rng = np.random.default_rng(8)
    C0 = np.asfortranarray(rng.integers(-3, 4, size=(m + 2, n)).astype(T))
    # k = 0, beta = 2: C = 2 C0, A and B never read (NULL)
    Cd = eu.DeviceArray.from_host(C0, ctx)
    assert _gemm(eu, ctx, T, m, n, 0, 1, None, m, None, 1, 2, Cd, m + 2) == OK
    ctx.sync()
    got = Cd.to_host()
    assert np.array_equal(got[:m], 2 * C0[:m]) and np.array_equal(got[m:], C0[m:])
    # k = 0, beta = 0: C = 0 whatever it held
    Cd = eu.DeviceArray.from_host(np.full((m + 2, n), np.nan, dtype=T, order="F"), ctx)
    assert _gemm(eu, ctx, T, m, n, 0, 1, None, m, None, 1, 0, Cd, m + 2) == OK
    ctx.sync()
    got = Cd.to_host()
    assert np.array_equal(got[:m], np.zeros((m, n), dtype=T)) and np.all(np.isnan(got[m:]))
    # m = 0 or n = 0: nothing is written
    Ad, Bd = eu.DeviceArray.from_host(np.ones((m, 4), dtype=T), ctx), eu.DeviceArray.from_host(np.ones((4, n), dtype=T), ctx)
    Cd = eu.DeviceArray.from_host(C0, ctx)
    assert _gemm(eu, ctx, T, 0, n, 4, 1, Ad, m, Bd, 4, 0, Cd, m + 2) == OK
    assert _gemm(eu, ctx, T, m, 0, 4, 1, Ad, m, Bd, 4, 0, Cd, m + 2) == OK
    ctx.sync()
    assert np.array_equal(Cd.to_host(), C0)


@pytest.mark.parametrize("m", [4096, 4095])
def test_product_on_both_sides_of_the_size_selected_tile(eu, tile_ctx, m):
    """float32 on a default context: m n = 4096^2 is GEMM_BIG_TILE_MIN_OUTPUTS (the big tile by size), 4095 x 4096 one row below it.
    Which tile ran cannot be seen from here; that the size-selected path is right on both sides of the switch can."""
    src = open(os.path.join(ROOT, "exponentialutilities.jl_amd", "csrc", "dense_dev.hip")).read()
    assert "GEMM_BIG_TILE_MIN_OUTPUTS = (int64_t)4096 * 4096;" in src
    ctx, n, k = tile_ctx["by_size"], 4096, 16
    rng = np.random.default_rng(m)
    A = np.asfortranarray(rng.integers(-3, 4, size=(m, k)).astype(np.float32))
    B = np.asfortranarray(rng.integers(-3, 4, size=(k, n)).astype(np.float32))
    Ad, Bd = eu.DeviceArray.from_host(A, ctx), eu.DeviceArray.from_host(B, ctx)
    Cd = eu.DeviceArray((m, n), np.float32, ctx)
    assert _gemm(eu, ctx, np.float32, m, n, k, 1, Ad, m, Bd, k, 0, Cd, m) == OK
    ctx.sync()
    assert np.array_equal(Cd.to_host(), A @ B)           # |entries| <= 144: exact in float32 in any order
