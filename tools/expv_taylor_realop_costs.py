"""What exp(-i tau A)b costs on a REAL operator by eu.expv_taylor_realop beside eu.expv_taylor on the promoted complex operator.

    python tools/expv_taylor_realop_costs.py [--out FILE] [--quick]

n = 10^6, a 5-diagonal operator (general diagonal form) and 8 random entries per row (SELL slots), Float64 and Float32, t purely
imaginary with alpha = |t| opnorm(A - mu I, Inf) = 40, complex vectors on the device.  Three calls, interleaved (a, b, c, a, b, c,
...), 2 warm-up rounds and the median [min .. max] of 7 timed ones, each call complete on return:
    (a) expv_taylor_realop on the real operator;
    (b) expv_taylor on the operator promoted to the complex type, built once outside the timing;
    (c) the Krylov expv (m = 30, tol 1e-7) on the promoted operator with the same t -- what 31 applications cost; at alpha = 40 a
        single Krylov space does not answer the same question (dist says how far it is).
Per call: ms, term launches, microseconds per term launch from the context's profiler (a separate, untimed call with the profiler
on), and (a) == (b) element for element.  Per operator: the creation time of the promoted copy and the device memory both operators
take (the drop of free device memory around the creation).  Expectation from counting bytes per row and term: 5 diagonals 104 B
against 144 B (0.72), 9 SELL entries 172 B against 244 B (0.70), in Float64.  These are measurements, not targets."""
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


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def created(make, ctx):
    ctx.sync()
    f0, t0 = free_bytes(), time.perf_counter()
    op = make()
    ctx.sync()
    return op, 1e3 * (time.perf_counter() - t0), f0 - free_bytes()


def term_us(call, ctx):
    """microseconds per term launch of the fused kernel, from the profiler, in a call of its own"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    ctx.sync()
    p = ctx.prof_get().get("matvec")
    ctx.prof_enable(False)
    return 1e3 * p["total_ms"] / p["launches"] if p else float("nan")


def relmax(a, b):
    d = float(b.abs().max())
    return float((a - b).abs().max()) / (d if d > 0 else 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expv_taylor_realop_costs.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 10^5, 3 timed rounds")
    a = ap.parse_args()
    n, warm, reps = (100_000, 1, 3) if a.quick else (1_000_000, 2, 7)
    ctx = eu.default_context()
    lines = ["# expv_taylor_realop (real operator, complex vectors) beside expv_taylor on the promoted operator and the Krylov expv: n = %d, t = -i tau," % n,
             "# alpha = %.0f, vectors on the device; ms per call = median [min .. max] of %d interleaved rounds; us/term = profiler time per fused term launch" % (ALPHA, reps)]
    for name, A64 in (("5 diagonals", c2_operator(n)), ("random sparse, 8 per row", random_sparse(n))):
        for R, Cd in ((np.float64, np.complex128), (np.float32, np.complex64)):
            A = A64.astype(R)
            rows = abs(A64 - sp.identity(n, format="csr") * (A64.diagonal().sum() / n)).sum(axis=1)
            t = -1j * ALPHA / float(np.asarray(rows).max())
            op, ms_r, bytes_r = created(lambda: eu.MIOperator(A, ctx), ctx)
            opc, ms_c, bytes_c = created(lambda: op.astype(Cd), ctx)
            b = torch.as_tensor(np.random.default_rng(3).standard_normal(n).astype(R) + 1j * np.random.default_rng(4).standard_normal(n).astype(R)).cuda()
            calls = {"realop": lambda: eu.expv_taylor_realop(t, op, b, return_info=True),
                     "promoted": lambda: eu.expv_taylor(t, opc, b, return_info=True),
                     "krylov 1e-7": lambda: (eu.expv(t, opc, b, m=30, tol=1e-7), None)}
            ts = {k: [] for k in calls}
            out = {}
            for i in range(warm + reps):
                for k, f in calls.items():      # interleaved: a, b, c, a, b, c, ...
                    ctx.sync()
                    t0 = time.perf_counter()
                    out[k] = f()
                    ctx.sync()
                    if i >= warm:
                        ts[k].append(1e3 * (time.perf_counter() - t0))
            us = {"realop": term_us(calls["realop"], ctx), "promoted": term_us(calls["promoted"], ctx), "krylov 1e-7": float("nan")}
            wa, wb = out["realop"][0], out["promoted"][0]
            med = {k: float(np.median(v)) for k, v in ts.items()}
            lines += ["", "## %s, %s: nnz = %d; real operator %.1f MB (created in %.0f ms), promoted copy %.1f MB more (made in %.0f ms)"
                      % (name, np.dtype(R).name, A.nnz, bytes_r / 1e6, ms_r, bytes_c / 1e6, ms_c),
                      "%-12s %-30s %8s %5s %9s %9s" % ("call", "ms per call", "launches", "path", "us/term", "dist")]
            for k in calls:
                v = np.array(ts[k])
                w, info = out[k]
                lines.append("%-12s %-30s %8s %5s %9.1f %9.2e" % (k, "%8.2f [%7.2f .. %7.2f]" % (np.median(v), v.min(), v.max()),
                                                                  info["launches"] if info else "-", info["path"] if info else "-", us[k], relmax(w, wa)))
            lines.append("realop / promoted: %.3f in ms per call, %.3f in us per term; realop == promoted: %s"
                         % (med["realop"] / med["promoted"], us["realop"] / us["promoted"], bool(torch.equal(wa, wb))))
            print("\n".join(lines[-6:]), flush=True)
            del op, opc
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
