"""What a block of columns costs by the truncated Taylor series: eu.expv_taylor_block beside one eu.expv_taylor call per column.

    python tools/expv_taylor_block_costs.py [--out FILE] [--quick]

The two operators of tools/expv_taylor_costs.py at n = 10^6 in Float64 (5 constant diagonals: general diagonal form; 8 random entries
per row + the diagonal: SELL slots), a random block on the device (a contiguous torch (n, p) tensor: row-major, no transpose),
alpha = |t| opnorm(A - mu I, Inf) in {3, 10}, p in {2, 4, 8, 16}.  Per point, wall-clock milliseconds (2 warm-ups, 5 timed, each
complete on return; median [min .. max]) of
    block   one expv_taylor_block call,
    loop    p expv_taylor calls on the columns (contiguous device vectors) -- the only way to do it before the block call,
with the operator applications (summed over the columns) and the term launches of each, and ratio = median(block) / min(loop).
Traffic model for the 5-diagonal operator, bytes per row and column: 80 for a single call (40 of the operator + 4 vector streams +
the cached gather), (40 + 8 * 40) / 8 = 45 for a block call at p = 8: a ratio of 0.56.  The bar: at p = 8 the block's median is below
the minimum of the loop on both operators; the script exits 1 when it is not."""
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
NCOLS = (2, 4, 8, 16)


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expv_taylor_block_costs.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 10^5")
    a = ap.parse_args()
    n = 100_000 if a.quick else 1_000_000
    ctx = eu.default_context()
    lines = ["# expv_taylor_block beside a loop of expv_taylor calls: n = %d, Float64, block on the device (row-major); ms = median [min .. max] of 5" % n,
             "# apps = operator applications summed over the columns, launches = term launches enqueued, ratio = median(block) / min(loop)"]
    missed = []
    for name, A in (("5 diagonals (headline)", c2_operator(n)), ("random sparse, 8 per row", random_sparse(n))):
        op = eu.MIOperator(A, ctx)
        rows = abs(A - sp.identity(n, format="csr") * (A.diagonal().sum() / n)).sum(axis=1)
        base = float(np.asarray(rows).max())
        lines += ["", "## %s: nnz = %d, opnorm(A - mu I, Inf) = %.4f" % (name, A.nnz, base),
                  "%7s %5s %-7s %-30s %7s %8s %5s %6s" % ("alpha", "ncols", "method", "ms", "apps", "launches", "path", "ratio")]
        for alpha in ALPHAS:
            t = alpha / base
            for p in NCOLS:
                B = torch.as_tensor(np.random.default_rng(3).standard_normal((n, p))).cuda()
                cols = [B[:, k].contiguous() for k in range(p)]

                def loop():
                    out = [eu.expv_taylor(t, op, c, return_info=True) for c in cols]
                    return torch.stack([w for w, _ in out], dim=1), [i for _, i in out]
                tb, (Wb, ib) = timed(lambda: eu.expv_taylor_block(t, op, B, return_info=True), ctx, 2, 5)
                tl, (Wl, il) = timed(loop, ctx, 2, 5)
                if not torch.equal(Wb, Wl):
                    raise SystemExit("%s, alpha %g, ncols %d: the block call and the loop differ" % (name, alpha, p))
                ratio = float(np.median(tb) / tl.min())
                lines.append("%7.0f %5d %-7s %-30s %7d %8d %5d %6.2f" % (alpha, p, "block", fmt(tb), ib["applications_total"], ib["launches"], ib["path"], ratio))
                lines.append("%7.0f %5d %-7s %-30s %7d %8d %5d" % (alpha, p, "loop", fmt(tl), sum(i["applications"] for i in il),
                                                                   sum(i["launches"] for i in il), il[0]["path"]))
                if p == 8 and not np.median(tb) < tl.min():
                    missed.append("%s, alpha %g: block %.2f ms, fastest loop %.2f ms" % (name, alpha, np.median(tb), tl.min()))
                print("\n".join(lines[-2:]), flush=True)
    lines += ["", "# bar (ncols = 8: median(block) < min(loop) on both operators): " + ("met" if not missed else "MISSED -- " + "; ".join(missed))]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
