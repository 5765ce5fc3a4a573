"""What the power-norm parameter search costs and when it pays, measured on the device at n = 10^6 -> profiles/normest_costs.txt.

  1. The eight estimates d_2 .. d_9 of expv_taylor_power (MIOperator.norm_power, p = 2 .. 9, infinity norm, adjoint given), in units of
     ONE term launch of expv_taylor on the same operator, for the 5-diagonal operator (fused panel kernel on the general diagonal
     form) and for 8 random entries per row (fused panel kernel on SELL slots).  A term launch = wall time of a warmed expv_taylor call
     that ends in its state read-back, over the launches it enqueued.
  2. On block-triangular operators [[L, c C], [0, L]] of order 10^6 (L the 1-D Laplacian, C as in tests/normest_cases.py without its
     10^3), the coupling c swept: wall time of expv_taylor and of expv_taylor_power (estimates included, adjoint given) -- the alpha_1
     at which the second starts to win.

Host clock around calls that end in a device synchronisation; every shape warmed; the median of REPS.  Needs a GPU."""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 5


def median_ms(f):
    f()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def five_diagonal(n):
    r = np.random.default_rng(5)
    coef = {-2: 0.3, -1: 1.2, 0: -2.0, 1: 0.8, 2: -0.1}
    return sp.diags([(0.5 + r.random(n - abs(o))) * c for o, c in coef.items()], list(coef), shape=(n, n), format="csr")


def random8(n):
    r = np.random.default_rng(8)
    cols = r.integers(0, n, size=(n, 8))
    vals = r.standard_normal((n, 8)) / np.sqrt(8.0)
    A = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, 8 * n + 1, 8)), shape=(n, n)) - sp.identity(n, format="csr")
    A.sum_duplicates()
    A.sort_indices()
    return A.tocsr()


def block_triangular(m, c):
    r = np.random.default_rng(1)
    L = sp.diags([np.ones(m - 1), -2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csr")
    Cc = sp.diags([c * (1 + r.random(m)), -0.5 * c * (1 + r.random(m - 1))], [0, 1], format="csr")
    A = sp.bmat([[L, Cc], [None, L]], format="csr")
    A.sort_indices()
    return A.tocsr()


def main():
    import expv_mi_loader
    eu = expv_mi_loader.load()
    n = 10 ** 6
    lines = ["# tools/normest_costs.py: n = %d, float64, host clock around synchronising calls, median of %d (min .. max)" % (n, REPS), ""]
    lines.append("# 1. the eight estimates (p = 2 .. 9) against one term launch of expv_taylor on the same operator")
    lines.append("%-14s %12s %14s %22s %12s %10s %8s" % ("operator", "term [us]", "estimates [ms]", "(min .. max)", "in terms", "panel apps", "reads"))
    for name, A in (("5-diagonal", five_diagonal(n)), ("random8", random8(n))):
        op = eu.MIOperator(A)
        adj = op.adjoint()
        b = np.random.default_rng(0).standard_normal(n)
        mu = float(A.diagonal().mean())
        t = 40.0 / float(abs(A - mu * sp.identity(n)).sum(axis=1).max())
        _, info = eu.expv_taylor(t, op, b, return_info=True)
        call_ms, _, _ = median_ms(lambda: eu.expv_taylor(t, op, b))
        term_us = 1e3 * call_ms / info["launches"]
        apps = reads = 0
        for p in range(2, 10):
            _, i = op.norm_power(p, np.inf, mu, adj, return_info=True)
            apps += i["applications"]
            reads += i["host_reads"]
        est_ms, lo, hi = median_ms(lambda: [op.norm_power(p, np.inf, mu, adj) for p in range(2, 10)])
        lines.append("%-14s %12.2f %14.3f %22s %12.1f %10d %8d" % (name, term_us, est_ms, "(%.3f .. %.3f)" % (lo, hi), 1e3 * est_ms / term_us, apps, reads))
    lines += ["", "# 2. block-triangular [[L, c C], [0, L]], n = %d, t = 1: expv_taylor against expv_taylor_power (estimates included)" % n]
    lines.append("%8s %10s %16s %12s %16s %12s %8s" % ("c", "alpha_1", "first (m*, s)", "first [ms]", "power (m*, s)", "power [ms]", "winner"))
    cross = None
    for c in (15.0, 20.0, 30.0, 50.0, 100.0, 300.0, 1000.0):
        A = block_triangular(n // 2, c)
        op = eu.MIOperator(A)
        adj = op.adjoint()
        b = np.random.default_rng(0).standard_normal(n)
        _, i1 = eu.expv_taylor(1.0, op, b, return_info=True)
        _, i2 = eu.expv_taylor_power(1.0, op, b, adjoint=adj, return_info=True)
        t1, _, _ = median_ms(lambda: eu.expv_taylor(1.0, op, b))
        t2, _, _ = median_ms(lambda: eu.expv_taylor_power(1.0, op, b, adjoint=adj))
        win = "power" if t2 < t1 else "first"
        if cross is None and i2["p_used"] and t2 < t1:
            cross = i1["alpha"]
        lines.append("%8.0f %10.1f %16s %12.2f %16s %12.2f %8s" % (c, i1["alpha"], "(%d, %d)" % (i1["m"], i1["s"]), t1, "(%d, %d) p=%d" % (i2["m"], i2["s"], i2["p_used"]), t2, win))
        del op, adj
    lines.append("# expv_taylor_power is the faster call from alpha_1 = %s on (the smallest swept alpha_1 above the cheap threshold at which it won)"
                 % ("%.1f" % cross if cross is not None else "none of the swept values"))
    out = os.path.join(ROOT, "profiles", "normest_costs.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
