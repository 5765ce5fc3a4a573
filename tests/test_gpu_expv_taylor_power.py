"""exp(tA)b by the truncated Taylor series with the reference's whole parameter search (expv_mi_expv_taylor_power,
eu.expv_taylor_power): the power norms d_2 .. d_9 from the estimator on the device, (m*, s) from host_taylor_params_power, the
series of expv_taylor behind them.

Bars.  d_p = |t| est_p^(1/p): the estimator's bar 8 p r eps || |B|^p || on est_p (tests/test_gpu_normest.py) carried through the root,
d_p / p times the relative bar.  Values: the bar of tests/test_gpu_expv_taylor.py, device error <= 8 x max(error of the numpy
restatement of the series in the operator's element type with the same (m*, s), eps_T), relative in the max norm.  Truth at order
200: scipy.linalg.expm(tA) b in 64-bit arithmetic; at order 1537 (where a dense expm is out of a test's reach): the first-branch
series run in longdouble, whose truncation error is below 2^-53 by the reference's own analysis."""
import os
import warnings

import numpy as np
import pytest
import scipy.linalg as sl

from tests import expv_taylor_cases as tc
from tests import normest_cases as nc

pytestmark = pytest.mark.gpu
BAR = 8.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_memo, _lines = {}, []


def note(line):
    _lines.append(line)
    print("[taylor_power]", line)


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    if not _lines:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "expv_taylor_power_parity.txt"), "w") as f:
            f.write("# expv_taylor_power on the device: parameters, applications and relative max-norm errors (tests/test_gpu_expv_taylor_power.py)\n")
            f.write("\n".join(_lines) + "\n")
    except OSError as e:
        warnings.warn("profiles/expv_taylor_power_parity.txt was not written: %s" % e)


@pytest.fixture(scope="module")
def eu():
    import expv_mi_loader
    return expv_mi_loader.load()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tables(eu):
    return {p: [eu.host_taylor_theta(m, p) for m in range(1, tc.M_MAX + 1)] for p in (0, 1)}


def bt(m, T):
    """the block-triangular operator in element type T (complex: turned by 0.6 + 0.8i, so that mu and the series are complex)"""
    A = nc.block_triangular(m, np.float64)
    if np.dtype(T).kind == "c":
        A = A * (0.6 + 0.8j)
    return A.astype(T).tocsr()


def memo(key, f):
    if key not in _memo:
        _memo[key] = f()
    return _memo[key]


def check_parameters(eu, A, t, info, precision, d_bar=True):
    """(m*, s) are the search's for the call's own d, and (d_bar: where dense powers are cheap) those d are the restated ones within
    the estimator's bar"""
    tab = tc.table_of(A.dtype, precision)
    mu = nc.mean_diagonal(A)
    assert (info["m"], info["s"], info["p_used"]) == eu.host_taylor_params_power(info["alpha"], info["d"], tab)
    assert info["normest_reads"] <= 2 * 5 * 8 and info["normest_applications"] > 0
    if not d_bar:
        return
    key = ("d", A.shape[0], A.dtype.name)
    d_rest, ex = memo(key, lambda: (nc.restated_d(A, 1.0, mu), nc.exact_norms(key, A, mu, ps=tuple(range(2, 10)))))
    r, eps = nc.longest_row(A), float(np.finfo(A.dtype).eps)
    for i, p in enumerate(range(2, 10)):
        dr = abs(t) * d_rest[i]
        rel = 8 * p * r * eps * ex[p][2] / (dr / abs(t)) ** p
        assert abs(info["d"][i] - dr) <= dr / p * rel * 1.01, (p, info["d"][i], dr, rel)


def test_block_triangular_1537_needs_a_twentieth_of_the_applications(eu, tables):
    A, mu = nc.case("bt1537")
    n, t = A.shape[0], 1.0
    b = tc.vector(n, np.float64)
    op = eu.MIOperator(A)
    adj = op.adjoint()
    w1, i1 = eu.expv_taylor(t, op, b, return_info=True)
    w, info = eu.expv_taylor_power(t, op, b, adjoint=adj, return_info=True)
    w, w1 = np.asarray(w), np.asarray(w1)
    note("bt1537: first branch (%d, %d) %d applications; power norms (%d, %d) p = %d, %d applications, %d estimator applications, %d reads"
          % (i1["m"], i1["s"], i1["applications"], info["m"], info["s"], info["p_used"], info["applications"], info["normest_applications"], info["normest_reads"]))
    assert info["m"] * info["s"] <= 60 and i1["m"] * i1["s"] >= 10 ** 4
    assert info["applications"] * 20 <= i1["applications"], (info, i1)
    assert info["alpha"] == i1["alpha"] and info["mu"] == i1["mu"]
    assert info["temporary_adjoint"] == 0 and info["host_reads"] <= 2
    check_parameters(eu, A, t, info, 0, d_bar=False)
    assert (info["m"], info["s"], info["p_used"]) == eu.host_taylor_params_power(info["alpha"], nc.restated_d(A, t, mu), 0)      # (the d bar: at order 200)
    truth, _ = nc.restated_series(t, A, b, i1["m"], i1["s"], mu, tc.TOL[0], arith=np.longdouble)
    e_rest = max(tc.relmax(nc.restated_series(t, A, b, m, s, mu, tc.TOL[0])[0], truth) for m, s in ((info["m"], info["s"]), (i1["m"], i1["s"])))
    bar = BAR * max(e_rest, tc.eps_of(np.float64))
    note("bt1537: |w_power - w_first| = %.2e, restated series %.2e, bar %.2e" % (tc.relmax(w, w1), e_rest, bar))
    assert tc.relmax(w, w1) <= bar


@pytest.mark.parametrize("T,precision", [(np.float64, 0), (np.complex128, 0), (np.float32, 0), (np.float64, 1)], ids=["f64", "c128", "f32", "f64-p1"])
def test_block_triangular_200_against_expm(eu, tables, T, precision):
    A = bt(200, T)
    n, t = A.shape[0], 1.0
    mu = nc.mean_diagonal(A)
    b = tc.vector(n, T)
    tab = tc.table_of(T, precision)
    w, info = eu.expv_taylor_power(t, A, b, precision=precision, return_info=True)
    w = np.asarray(w)
    assert w.dtype == np.dtype(T) and info["temporary_adjoint"] == 1 and info["p_used"] >= 2
    check_parameters(eu, A, t, info, precision)
    W = tc.wide(T)
    truth = sl.expm(t * A.toarray().astype(W)) @ b.astype(W)
    Fr, apps = nc.restated_series(t, A, b, info["m"], info["s"], mu, tc.TOL[tab])
    e_rest, e_dev = tc.relmax(Fr, truth), tc.relmax(w, truth)
    note("bt200 %-10s precision %d: (m*, s) = (%d, %d) p = %d, %d applications; restated %.2e device %.2e"
          % (np.dtype(T).name, precision, info["m"], info["s"], info["p_used"], info["applications"], e_rest, e_dev))
    assert abs(info["applications"] - apps) <= info["s"]
    assert e_dev <= BAR * max(e_rest, tc.eps_of(T)), (e_dev, e_rest)
    m1, s1 = eu.host_taylor_params(info["alpha"], tab)
    assert info["m"] * info["s"] * 20 <= m1 * s1


@pytest.mark.parametrize("T", [np.float64, np.complex64])
def test_below_the_cheap_threshold_the_call_is_expv_taylor(eu, tables, T):
    n = 1000
    A, b = tc.random8(n, T), tc.vector(n, T)
    tab = tc.table_of(T, 0)
    cheap = 4 * tables[tab][54] * 8 * 11 / 55
    t = tc.t_for(A, 0.9 * cheap)
    op = eu.MIOperator(A)
    w1, i1 = eu.expv_taylor(t, op, b, return_info=True)
    w, info = eu.expv_taylor_power(t, op, b, return_info=True)
    assert info["alpha"] <= cheap
    assert np.array_equal(np.asarray(w).view(np.uint8), np.asarray(w1).view(np.uint8))
    assert (info["p_used"], info["normest_applications"], info["normest_reads"], info["temporary_adjoint"]) == (0, 0, 0, 0)
    assert {k: info[k] for k in i1} == i1 and info["d"] == [0.0] * 8
    w0, i0 = eu.expv_taylor_power(0.0, op, b, return_info=True)
    assert np.array_equal(np.asarray(w0).view(np.uint8), b.view(np.uint8)) and (i0["m"], i0["s"], i0["normest_applications"]) == (0, 1, 0)


def test_max_matvecs_is_compared_with_the_refined_parameters(eu):
    A = bt(200, np.float64)
    n = A.shape[0]
    b = tc.vector(n, np.float64)
    op = eu.MIOperator(A)
    adj = op.adjoint()
    _, info = eu.expv_taylor_power(1.0, op, b, adjoint=adj, return_info=True)
    w = np.full(n, 7.0)
    with pytest.raises(eu.ExpvMIError, match=r"m\* = %d terms in each of s = %d stages, more than max_matvecs = %d" % (info["m"], info["s"], info["m"] * info["s"] - 1)):
        eu.expv_taylor_power_(w, 1.0, op, b, adjoint=adj, max_matvecs=info["m"] * info["s"] - 1)
    assert np.all(w == 7.0)
    eu.expv_taylor_power_(w, 1.0, op, b, adjoint=adj, max_matvecs=info["m"] * info["s"])      # (the first branch would need 16 280)
    assert np.array_equal(w, np.asarray(eu.expv_taylor_power(1.0, op, b, adjoint=adj)))
    with pytest.raises(eu.ExpvMIError):
        eu.expv_taylor(1.0, op, b, max_matvecs=info["m"] * info["s"])


def test_argument_errors(eu):
    A = bt(200, np.float64)
    n = A.shape[0]
    b = tc.vector(n, np.float64)
    op = eu.MIOperator(A)
    with pytest.raises(eu.ExpvMIError, match="dtype or n"):
        eu.expv_taylor_power(1.0, op, b, adjoint=eu.MIOperator(bt(100, np.float64)).adjoint())
    with pytest.raises(eu.ExpvMIError, match="another context"):
        eu.expv_taylor_power(1.0, op, b, adjoint=eu.MIOperator(A, eu.Context()).adjoint())
    with pytest.raises(eu.ExpvMIError):
        eu.expv_taylor_power(1.0, op, b, precision=2)
    with pytest.raises(eu.ExpvMIError):
        eu.expv_taylor_power(1.0 + 1.0j, op, b)
    Ad = A.toarray()
    mf = eu.MIOperator(None, matvec=lambda x: Ad @ x, shape=(n, n), dtype=np.float64, ishermitian=False)
    with pytest.raises(eu.ExpvMIError, match="matrix-free") as ei:
        eu.expv_taylor_power(1.0, mf, b)
    assert ei.value.kind == "Unsupported"


def test_host_and_device_vectors(eu, torch):
    A = bt(200, np.float64)
    n = A.shape[0]
    b = tc.vector(n, np.float64)
    op = eu.MIOperator(A)
    adj = op.adjoint()
    want, info = eu.expv_taylor_power(1.0, op, b, adjoint=adj, return_info=True)
    x = torch.as_tensor(b).cuda()
    wd = eu.expv_taylor_power(1.0, op, x, adjoint=adj)
    assert torch.is_tensor(wd) and wd.is_cuda and np.array_equal(wd.cpu().numpy(), want)
    assert eu.expv_taylor_power.last_info == info
    out = eu.expv_taylor_power_(x, 1.0, op, x, adjoint=adj)      # b and w are the same device tensor
    assert out is x and np.array_equal(x.cpu().numpy(), want)
    wh = np.empty(n)
    eu.expv_taylor_power_(wh, 1.0, op, torch.as_tensor(b).cuda(), adjoint=adj)      # device b, host w
    assert np.array_equal(wh, want)
    bt_host = torch.as_tensor(b.copy())
    wt = eu.expv_taylor_power(1.0, op, bt_host, adjoint=adj)
    assert torch.is_tensor(wt) and not wt.is_cuda and np.array_equal(wt.numpy(), want)


def test_reordered_operator(eu, tables):
    """a block-triangular coupling of two shuffled bands, stored in the bandwidth-reducing ordering: the result comes back in the
    caller's numbering and the parameters are those of the unreordered operator"""
    import scipy.sparse as sp
    n0 = 500
    B, q = tc.shuffled_band(n0, np.float64)
    r = np.random.default_rng(2)
    Cc = sp.diags([300.0 * (1 + r.random(n0))], [0], format="csr")[q][:, q]
    A = sp.bmat([[B, Cc], [None, B]], format="csr").astype(np.float64).tocsr()
    A.sort_indices()
    n = A.shape[0]
    b = tc.vector(n, np.float64)
    mu = nc.mean_diagonal(A)
    ctx = eu.Context()
    ctx.set_option("reorder", 2)
    op = eu.MIOperator(A, ctx)
    assert op.reorder_info["reordered"]
    plain = eu.Context()
    plain.set_option("reorder", 0)
    p_op = eu.MIOperator(A, plain)
    w, info = eu.expv_taylor_power(1.0, op, b, return_info=True)
    wp, ip = eu.expv_taylor_power(1.0, p_op, b, return_info=True)
    assert info["p_used"] >= 2 and (info["m"], info["s"], info["p_used"]) == (ip["m"], ip["s"], ip["p_used"])
    m1, s1 = eu.host_taylor_params(info["alpha"], 0)
    truth, _ = nc.restated_series(1.0, A, b, m1, s1, mu, tc.TOL[0], arith=np.longdouble)
    e_rest = tc.relmax(nc.restated_series(1.0, A, b, info["m"], info["s"], mu, tc.TOL[0])[0], truth)
    bar = BAR * max(e_rest, tc.eps_of(np.float64))
    note("reordered: (m*, s) = (%d, %d) against (%d, %d); restated %.2e device %.2e" % (info["m"], info["s"], m1, s1, e_rest, tc.relmax(np.asarray(w), truth)))
    assert tc.relmax(np.asarray(w), truth) <= bar and tc.relmax(np.asarray(wp), truth) <= bar
