"""What exp(tA)b costs by the truncated Taylor series (eu.expv_taylor) beside the Krylov expv, as |t| ||A|| grows.

    python tools/expv_taylor_costs.py [--out FILE] [--quick]

Two operators of n = 10^6 in Float64, vectors on the device: the headline operator (5 constant diagonals, non-symmetric: general
diagonal form, fused term kernel) and a random sparse one (8 entries per row + the diagonal: SELL slots, fused term kernel).
t is chosen so that alpha = |t| opnorm(A - mu I, Inf) takes the values 1, 3, 10, 30, 100, 300, 1000.  Per point, wall-clock
milliseconds per call (2 warm-ups, 5 timed calls, each complete on return; median [min .. max]), operator applications made and
launches enqueued for
    expv_taylor at precision 0 (tol 2^-53) and 1 (the 2^-24 table, double arithmetic),
    expv(t, A, b; m = 30) at tol = 1e-7 and 1e-12 (31 applications of the operator each, whatever alpha is),
and the distance of each result from expv_taylor at precision 0, relative in the max norm: a single Krylov space of dimension 30
does NOT resolve a large alpha (the reference sub-steps with expv_timestep there), so the Krylov columns say what 31 applications
cost, and the distance says from which alpha on they no longer answer the same question.  These are measurements, not targets."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import expv_mi_loader
from tests._util import c2_operator

eu = expv_mi_loader.load()
ALPHAS = (1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1000.0)


def random_sparse(n, k=8, seed=7):
    r = np.random.default_rng(seed)
    cols = r.integers(0, n, size=(n, k))
    vals = r.standard_normal((n, k)) / np.sqrt(k)
    A = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n)) - sp.identity(n, format="csr")
    A.sum_duplicates()
    A.sort_indices()
    return A


def timed(f, ctx, warm, reps):
    ts, out = [], None
    for i in range(warm + reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = f()
        ctx.sync()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    ts = np.array(ts)
    return "%8.2f [%7.2f .. %7.2f]" % (np.median(ts), ts.min(), ts.max()), out


def relmax(a, b):
    d = float(b.abs().max())
    return float((a - b).abs().max()) / (d if d > 0 else 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expv_taylor_costs.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 10^5, alpha up to 100")
    a = ap.parse_args()
    n = 100_000 if a.quick else 1_000_000
    alphas = ALPHAS[:5] if a.quick else ALPHAS
    ctx = eu.default_context()
    lines = ["# expv_taylor beside expv (Krylov, m = 30): n = %d, Float64, vectors on the device; ms per call = median [min .. max] of 5" % n,
             "# apps = operator applications, launches = term launches enqueued (expv_taylor) ; dist = |w - w_taylor53|_inf / |w_taylor53|_inf"]
    for name, A in (("5 diagonals (headline)", c2_operator(n)), ("random sparse, 8 per row", random_sparse(n))):
        op = eu.MIOperator(A, ctx)
        b = torch.as_tensor(np.random.default_rng(3).standard_normal(n)).cuda()
        rows = abs(A - sp.identity(n, format="csr") * (A.diagonal().sum() / n)).sum(axis=1)
        base = float(np.asarray(rows).max())
        lines += ["", "## %s: nnz = %d, opnorm(A - mu I, Inf) = %.4f" % (name, A.nnz, base),
                  "%7s %-10s %-30s %6s %8s %5s %9s" % ("alpha", "method", "ms per call", "apps", "launches", "path", "dist")]
        for alpha in alphas:
            t = alpha / base
            ref = None
            for label, f in (("taylor 53", lambda: eu.expv_taylor(t, op, b, precision=0, return_info=True)),
                             ("taylor 24", lambda: eu.expv_taylor(t, op, b, precision=1, return_info=True)),
                             ("krylov 1e-7", lambda: (eu.expv(t, op, b, m=30, tol=1e-7), None)),
                             ("krylov 1e-12", lambda: (eu.expv(t, op, b, m=30, tol=1e-12), None))):
                ms, (w, info) = timed(f, ctx, 2, 5)
                if ref is None:
                    ref = w
                if info is not None:
                    apps, launches, path = info["applications"], info["launches"], info["path"]
                else:
                    st = eu.expv.last_stats
                    apps, launches, path = st["matvecs"], "-", "+".join(st["path"])
                lines.append("%7.0f %-12s %-30s %6s %8s %5s %9.2e" % (alpha, label, ms, apps, launches, path, relmax(w, ref)))
            print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
