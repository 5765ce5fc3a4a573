"""What sum_k t^k phi_k(tA) u_k costs without a Krylov basis: eu.phiv_taylor beside eu.phiv_timestep on the same inputs.

    python tools/phiv_taylor_costs.py [--out FILE] [--quick]

The two operators of tools/expv_taylor_costs.py at n = 10^6 in Float64 (5 constant diagonals: general diagonal form; 8 random entries
per row + the diagonal: SELL slots), B = [u_0 ... u_p] a random column-major block on the device, p in {1, 3},
|t| opnorm(A - mu I, Inf) in {3, 10}.  Per point, wall-clock milliseconds (2 warm-ups, 5 timed, each complete on return; median
[min .. max]) of
    taylor53   phiv_taylor at the working precision (tol 2^-53),
    taylor24   phiv_taylor with precision = 1 (the 2^-24 table: the tolerance class of the Krylov call),
    krylov     phiv_timestep(t, A, B) with its defaults (tol 1e-7, m = 30, adaptive sub-steps),
with the operator applications of each and the relative max-norm difference of each from taylor53.  Nothing is asserted: the file
records where the series wins and where it loses."""
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
from tools.expv_taylor_costs import random_sparse

eu = expv_mi_loader.load()
ALPHAS = (3.0, 10.0)
PS = (1, 3)


def timed(f, ctx, warm, reps):
    ts, out = [], None
    for i in range(warm + reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = f()
        ctx.sync()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return np.array(ts), out


def fmt(ts):
    return "%8.2f [%7.2f .. %7.2f]" % (np.median(ts), ts.min(), ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "phiv_taylor_costs.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 10^5")
    a = ap.parse_args()
    n = 100_000 if a.quick else 1_000_000
    ctx = eu.default_context()
    lines = ["# phiv_taylor beside phiv_timestep: n = %d, Float64, column-major block on the device; ms = median [min .. max] of 5" % n,
             "# apps = operator applications (taylor: terms that entered F; krylov: matvecs), diff = relative max-norm difference from taylor53,",
             "# ratio = median(method) / median(krylov)"]
    for name, A in (("5 diagonals (headline)", c2_operator(n)), ("random sparse, 8 per row", random_sparse(n))):
        op = eu.MIOperator(A, ctx)
        for p in PS:
            mu = A.diagonal().sum() / (n + p)
            base = float(np.asarray(abs(A - sp.identity(n, format="csr") * mu).sum(axis=1)).max())
            lines += ["", "## %s, p = %d: nnz = %d, opnorm(A - mu I, Inf) = %.4f" % (name, p, A.nnz, base),
                      "%7s %-9s %-30s %7s %5s %5s %10s %6s" % ("alpha", "method", "ms", "apps", "m*", "s", "diff", "ratio")]
            B = torch.as_tensor(np.random.default_rng(3).standard_normal((p + 1, n))).cuda().t()      # column-major n x (p + 1)
            for alpha in ALPHAS:
                t = alpha / base
                st = {}
                tk, wk = timed(lambda: eu.phiv_timestep(t, op, B, stats=st), ctx, 2, 5)
                t53, (w53, i53) = timed(lambda: eu.phiv_taylor(t, op, B, return_info=True), ctx, 2, 5)
                t24, (w24, i24) = timed(lambda: eu.phiv_taylor(t, op, B, precision=1, return_info=True), ctx, 2, 5)
                ref = w53.cpu().numpy()
                diff = lambda w: float(np.max(np.abs(np.asarray(w.cpu().numpy() if torch.is_tensor(w) else w).ravel() - ref)) / np.max(np.abs(ref)))
                mk = float(np.median(tk))
                for meth, ts, w, apps, m, s in (("taylor53", t53, w53, i53["applications"], i53["m"], i53["s"]),
                                                ("taylor24", t24, w24, i24["applications"], i24["m"], i24["s"]),
                                                ("krylov", tk, wk, st.get("matvecs", -1), 0, 0)):
                    lines.append("%7.0f %-9s %-30s %7d %5d %5d %10.2e %6.2f" % (alpha, meth, fmt(ts), apps, m, s, diff(w), float(np.median(ts)) / mk))
                print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
