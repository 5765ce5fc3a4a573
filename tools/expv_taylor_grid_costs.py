"""What snapshots cost by the truncated Taylor series: one eu.expv_taylor_grid call beside the ways to get them without it.

    python tools/expv_taylor_grid_costs.py [--out FILE] [--quick]

The two operators of tools/expv_taylor_costs.py at n = 10^6 in Float64 (5 constant diagonals: general diagonal form; 8 random entries
per row + the diagonal: SELL slots), a random vector on the device, alpha = |T| opnorm(A - mu I, Inf) = 40, q in {8, 64} equally
spaced outputs ts = T k / q.  Per point, wall-clock milliseconds (2 warm-ups, 5 timed, each complete on return; median [min .. max]) of
    grid      one expv_taylor_grid call (results in a torch (n, q) device tensor),
    (a) T     the single expv_taylor call to T alone: what the grid's outputs cost on top of it,
    (b) each  q expv_taylor calls, one per output, each from b,
    (c) chain q expv_taylor calls from output to output (Al-Mohy & Higham's Algorithm 5.2 in spirit),
    (d) krylov expv_timestep(ts, A, b) with the tolerance of the same class (precision 0: tol 1e-12, precision 1: tol 1e-7),
with operator applications and term launches, the ratio of each median to the grid's, and the largest difference of (b), (c) and (d)
from the grid's outputs relative to the largest entry.  Traffic model of the fused term kernel with a panel of P interior outputs:
the operator and 4 vector streams (x, F read, y and F written) as the single call, plus 2 P streams (the panel read and written):
4 + 2 P streams of 8 n bytes beside the operator; the prediction for grid / (a) printed beside each point uses the mean P of the
stages of that grid.  A record, not a bar: nothing here was measured before this tool existed, and a loss is written down as such."""
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
ALPHA = 40.0
OUTPUTS = (8, 64)


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
    return "%9.2f [%8.2f .. %8.2f]" % (np.median(ts), ts.min(), ts.max())


def panel_width(c):
    return 0 if c == 0 else 2 if c <= 2 else 4 if c <= 4 else 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expv_taylor_grid_costs.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 10^5")
    a = ap.parse_args()
    n = 100_000 if a.quick else 1_000_000
    ctx = eu.default_context()
    lines = ["# expv_taylor_grid beside the single call, q single calls, q chained calls and the Krylov expv_timestep: n = %d, Float64, alpha = %g," % (n, ALPHA),
             "# vectors on the device; ms = median [min .. max] of 5; apps = operator applications, launches = term launches (+ accumulate-only ones),",
             "# x grid = median / median(grid); diff = largest difference from the grid's outputs / largest entry; model = predicted grid / (a) from",
             "# (operator + 4 + 2 P streams) / (operator + 4 streams) per term launch, P averaged over the stages (extra panels: 1 + 2 P streams each)"]
    for name, A, op_streams in (("5 diagonals (headline)", c2_operator(n), 5.0), ("random sparse, 8 per row", random_sparse(n), 9 * 1.5)):
        # operator bytes per row in units of one 8-byte vector stream: 5 diagonals of values; 9 slots of value + 4-byte column index
        op = eu.MIOperator(A, ctx)
        rows = abs(A - sp.identity(n, format="csr") * (A.diagonal().sum() / n)).sum(axis=1)
        base = float(np.asarray(rows).max())
        T = ALPHA / base
        b = torch.as_tensor(np.random.default_rng(3).standard_normal(n)).cuda()
        lines += ["", "## %s: nnz = %d, opnorm(A - mu I, Inf) = %.4f, T = %.4f" % (name, A.nnz, base, T),
                  "%4s %5s %-9s %-32s %6s %9s %7s %9s %6s" % ("prec", "q", "method", "ms", "apps", "launches", "x grid", "diff", "model")]
        for precision, ktol in ((0, 1e-12), (1, 1e-7)):
            for q in OUTPUTS:
                ts = T * np.arange(1, q + 1) / q

                def each():
                    out = [eu.expv_taylor(float(x), op, b, precision=precision, return_info=True) for x in ts]
                    return torch.stack([w for w, _ in out], dim=1), [i for _, i in out]

                def chain():
                    ws, infos, w, prev = [], [], b, 0.0
                    for x in ts:
                        w, i = eu.expv_taylor(float(x - prev), op, w, precision=precision, return_info=True)
                        ws.append(w)
                        infos.append(i)
                        prev = x
                    return torch.stack(ws, dim=1), infos

                def krylov():
                    st = {}
                    U = eu.expv_timestep(ts.copy(), op, b, tol=ktol, stats=st)
                    return U, st
                tg, (Wg, ig) = timed(lambda: eu.expv_taylor_grid(ts, op, b, precision=precision, return_info=True), ctx, 2, 5)
                t1, (_, i1) = timed(lambda: eu.expv_taylor(T, op, b, precision=precision, return_info=True), ctx, 2, 5)
                te, (We, ie) = timed(each, ctx, 2, 5)
                tc_, (Wc, ic) = timed(chain, ctx, 2, 5)
                tk, (Wk, sk) = timed(krylov, ctx, 2, 5)
                scale = float(Wg.abs().max())
                counts = {}
                for st_, kd in zip(ig["stage"], ig["kind"]):
                    if kd == 1:
                        counts[st_] = counts.get(st_, 0) + 1
                extra = 0.0
                for c in counts.values():
                    extra += 2 * panel_width(min(c, 8)) + sum(1 + 2 * panel_width(min(8, c - 8 * k)) for k in range(1, -(-c // 8)))
                model = (op_streams + 4 + extra / ig["s"]) / (op_streams + 4)
                gm = float(np.median(tg))

                def row(method, t, apps, launches, W=None, mdl=""):
                    diff = "" if W is None else "%9.2e" % (float((torch.as_tensor(W).to(Wg.device).reshape(Wg.shape) - Wg).abs().max()) / scale)
                    lines.append("%4d %5d %-9s %-32s %6s %9s %7.2f %9s %6s" % (precision, q, method, fmt(t), apps, launches, float(np.median(t)) / gm, diff, mdl))
                row("grid", tg, ig["applications"], "%d+%d" % (ig["launches"], ig["accumulate_launches"]))
                row("(a) T", t1, i1["applications"], i1["launches"], mdl="%.2f" % model)
                row("(b) each", te, sum(i["applications"] for i in ie), sum(i["launches"] for i in ie), We)
                row("(c) chain", tc_, sum(i["applications"] for i in ic), sum(i["launches"] for i in ic), Wc)
                row("(d) krylov", tk, sk.get("matvecs", sk.get("nmatvec", "-")), "-", Wk)
                lines.append("%4s %5s %-9s measured grid / (a) = %.2f" % ("", "", "", gm / float(np.median(t1))))
                print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
